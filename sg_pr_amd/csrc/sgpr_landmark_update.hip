// Folding further scans into a landmark map (sgpr_landmark_update; include/sgpr_landmark_update.h): a
// node that sgpr_landmark_align associated with a landmark becomes one more observation of its record, the nodes the map
// does not explain are fused among themselves into new landmarks behind the old ones.  HBM-bound integer work, no matrix
// cores.
//
//   upd_classify_kernel   one thread per node: the map point, live or dead; observation, new or rejected.  An observation
//                         adds its three fixed-point coordinates, a count and its session bit to the accumulators of its
//                         landmark (integer atomics: any order, same sums).  The masked label (the label of a new node,
//                         -1 of any other) and the landmark of an observation (-1 of any other) go to the workspace, so
//                         d_assoc is not read again and may be d_node_landmark.  Live nodes and observations are counted
//                         per wave, one atomic each.
//   upd_centre_kernel     one thread per old landmark with observations: S_k and center' into the workspace.
//   upd_spread_kernel     one thread per observation: its capped squared distance to center' into Q of its landmark.
//   lm_core_launch        sgpr_landmarks.hip's seven kernels on the masked labels (sgpr_landmark_core.hpp): the new
//                         landmarks, numbered from L, first from node_base, sessions shifted by session_base; it writes
//                         d_node_landmark of every node (-1 of those that are not new) and (L', new nodes).
//   upd_finish_kernel     one thread per old landmark: the parallel-axis term and the record, or the copy.  One thread
//                         also fills d_num.  Every thread reads its whole input record before it writes, and no kernel
//                         before this one writes a record below L: that is what makes the update in place safe.
//   upd_merge_kernel      one thread per node: an observation's d_node_landmark is its landmark.
//
// CONTENTION.  The atomics on one landmark's accumulators are bounded by the observations of one object - tens per drive
// - and there is no per-wave pre-reduction (cdna_hip_programming guideline 12: measured need first; the all-on-one case
// is tested for its bits, not tuned).
//
// The accumulators are zeroed by one memset on the stream; nothing else of the workspace is read before it is written.
// The eligible rule and the fixed-point constants are sgpr_map_grid.hpp's (record_eligible, MAP_FIX, MAP_D2_CAP), shared
// with sgpr_landmark_merge.hip.
// No floating-point atomics, no inline assembly, plain vector stores.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_core.hpp"
#include "sgpr_landmark_update.h"
#include "sgpr_map_grid.hpp"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

struct UpdWs {
    int* mlab;                     // [P] the label of a new node, -1 of any other
    int* obs;                      // [P] the landmark of an observation, -1 of any other
    // zeroed by the memset, one span:
    long long* sum;                // [L][3] fixed-point coordinate sums of the observations
    unsigned long long* q;         // [L] fixed-point sum of their squared distances to center'
    unsigned long long* sess;      // [L] their session bits
    int* cnt;                      // [L] n1
    int* tally;                    // [64] (live nodes, observations)
    // written before read:
    double* centre;                // [L][3] center'
    int* core_num;                 // [64] (L', new nodes) of the core
};

struct UpdArgs {
    const float* centers;
    const int32_t* labels;
    const double* poses;
    const int32_t* assoc;
    const double* lm_center;
    const int32_t* lm_label;
    const int32_t* lm_count;
    const int32_t* lm_first;
    const unsigned long long* lm_sessions;
    const double* lm_spread;
    double* out_center;
    int32_t* out_label;
    int32_t* out_count;
    int32_t* out_first;
    unsigned long long* out_sessions;
    double* out_spread;
    int32_t* node_landmark;
    int32_t* num;
    int P, N, L, n_labels, n_sessions, session_base;
    double radius[SGPR_LANDMARK_MAX_LABELS];
    int32_t starts[SGPR_SESSION_MAX];
};

// ELIGIBLE of the header, on the input record
__device__ __forceinline__ bool upd_eligible(const UpdArgs& a, int id) {
    const double* c = a.lm_center + 3 * (size_t)id;
    return record_eligible(a.lm_label[id], a.lm_count[id], a.lm_spread[id], c[0], c[1], c[2], a.radius, a.n_labels);
}

__global__ __launch_bounds__(LM_THREADS) void upd_classify_kernel(const UpdWs w, const UpdArgs a) {
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    bool live = false, seen = false;
    if (p < a.P) {
        const int q = p / a.N, l = a.labels[p];
        double m[3];
        live = lm_map_point(a.centers, a.poses, a.radius, a.n_labels, p, q, l, m);
        const int id = a.assoc[p];
        seen = live && id >= 0 && id < a.L && a.lm_label[id] == l && upd_eligible(a, id);
        w.mlab[p] = live && id == -2 ? l : -1;
        w.obs[p] = seen ? id : -1;
        if (seen) {
            for (int k = 0; k < 3; ++k)
                atomicAdd(reinterpret_cast<unsigned long long*>(&w.sum[3 * (size_t)id + k]), (unsigned long long)llrint(m[k] * MAP_FIX));
            atomicAdd(&w.cnt[id], 1);
            atomicOr(&w.sess[id], 1ull << (a.session_base + session_of(a.starts, a.n_sessions, q)));
        }
    }
    const unsigned long long lives = __ballot(live), sees = __ballot(seen);
    if ((threadIdx.x & 63) == 0) {
        if (lives) atomicAdd(&w.tally[0], __popcll(lives));
        if (sees) atomicAdd(&w.tally[1], __popcll(sees));
    }
}

__global__ __launch_bounds__(LM_THREADS) void upd_centre_kernel(const UpdWs w, const UpdArgs a) {
    const int id = blockIdx.x * LM_THREADS + threadIdx.x;
    if (id >= a.L) return;
    const int n1 = w.cnt[id];
    if (n1 == 0) return;                                        // (n1 > 0: the landmark is eligible)
    const double n0 = (double)a.lm_count[id], cnt = (double)(a.lm_count[id] + n1);
    for (int k = 0; k < 3; ++k) {
        const unsigned long long S = (unsigned long long)llrint((a.lm_center[3 * (size_t)id + k] * n0) * MAP_FIX) +
                                     (unsigned long long)w.sum[3 * (size_t)id + k];
        w.centre[3 * (size_t)id + k] = (double)(long long)S / (cnt * MAP_FIX);
    }
}

__global__ __launch_bounds__(LM_THREADS) void upd_spread_kernel(const UpdWs w, const UpdArgs a) {
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const int id = w.obs[p];
    if (id < 0) return;
    double m[3];
    lm_map_point(a.centers, a.poses, a.radius, a.n_labels, p, p / a.N, a.labels[p], m);
    const double ex = m[0] - w.centre[3 * (size_t)id], ey = m[1] - w.centre[3 * (size_t)id + 1];
    const double d2 = ex * ex + ey * ey;
    atomicAdd(&w.q[id], (unsigned long long)llrint(fmin(d2, MAP_D2_CAP) * MAP_FIX));
}

__global__ __launch_bounds__(LM_THREADS) void upd_finish_kernel(const UpdWs w, const UpdArgs a) {
    const int id = blockIdx.x * LM_THREADS + threadIdx.x;
    if (id == 0) {
        a.num[0] = w.core_num[0];
        a.num[1] = w.tally[0];
        a.num[2] = w.tally[1];
        a.num[3] = w.core_num[1];
    }
    if (id >= a.L) return;
    const double c0 = a.lm_center[3 * (size_t)id], c1 = a.lm_center[3 * (size_t)id + 1], c2 = a.lm_center[3 * (size_t)id + 2];
    const int label = a.lm_label[id], count = a.lm_count[id], first = a.lm_first[id];
    const unsigned long long sessions = a.lm_sessions[id];
    const double spread = a.lm_spread[id];
    const int n1 = w.cnt[id];
    a.out_label[id] = label;
    a.out_first[id] = first;
    if (n1 == 0) {
        a.out_center[3 * (size_t)id] = c0;
        a.out_center[3 * (size_t)id + 1] = c1;
        a.out_center[3 * (size_t)id + 2] = c2;
        a.out_count[id] = count;
        a.out_sessions[id] = sessions;
        a.out_spread[id] = spread;
        return;
    }
    const double n0 = (double)count, cnt = (double)(count + n1);
    const double d0 = w.centre[3 * (size_t)id], d1 = w.centre[3 * (size_t)id + 1], d2 = w.centre[3 * (size_t)id + 2];
    const double ax = c0 - d0, ay = c1 - d1;
    const double v = spread * spread + (ax * ax + ay * ay);
    const unsigned long long Q = (unsigned long long)llrint((fmin(v, MAP_D2_CAP) * n0) * MAP_FIX) + w.q[id];
    a.out_center[3 * (size_t)id] = d0;
    a.out_center[3 * (size_t)id + 1] = d1;
    a.out_center[3 * (size_t)id + 2] = d2;
    a.out_count[id] = count + n1;
    a.out_sessions[id] = sessions | w.sess[id];
    a.out_spread[id] = sqrt((double)Q / (cnt * MAP_FIX));
}

__global__ __launch_bounds__(LM_THREADS) void upd_merge_kernel(const UpdWs w, const UpdArgs a) {
    const int p = blockIdx.x * LM_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const int id = w.obs[p];
    if (id >= 0) a.node_landmark[p] = id;
}

size_t upd_zero_bytes(size_t L) { return align256(L * 24) + align256(L * 8) * 2 + align256(L * 4) + align256(64 * 4); }

size_t upd_ws_bytes(size_t P, size_t L) {
    return lm_core_workspace_bytes(P) + align256(P * 4) * 2 + upd_zero_bytes(L) + align256(L * 24) + align256(64 * 4);
}

bool upd_size_ok(int Q, int N, int L) {
    return Q >= 0 && N >= 0 && L >= 0 && (long long)Q * (long long)N <= (1ll << 30);
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_update_workspace_bytes(int Q, int N, int L) {
    if (!upd_size_ok(Q, N, L) || Q == 0 || N == 0) return 0;
    return upd_ws_bytes((size_t)Q * (size_t)N, (size_t)L);
}

int sgpr_landmark_update(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_poses,
                         const int32_t* d_assoc, const int32_t* h_starts, int n_sessions, int session_base, int node_base,
                         const double* h_radius, int n_labels, double tau_z, const double* d_lm_center,
                         const int32_t* d_lm_label, const int32_t* d_lm_count, const int32_t* d_lm_first,
                         const uint64_t* d_lm_sessions, const double* d_lm_spread, int L, int max_landmarks,
                         double* d_out_center, int32_t* d_out_label, int32_t* d_out_count, int32_t* d_out_first,
                         uint64_t* d_out_sessions, double* d_out_spread, int32_t* d_node_landmark, int32_t* d_num,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_update";
    if (!no_negative(fn, {{"Q", Q}, {"N", N}, {"L", L}, {"max_landmarks", max_landmarks}, {"node_base", node_base},
                          {"session_base", session_base}}))
        return SGPR_E_INVALID;
    if (max_landmarks < L) {
        set_error(fn + ": max_landmarks " + std::to_string(max_landmarks) + " is below L " + std::to_string(L));
        return SGPR_E_INVALID;
    }
    if (!landmark_labels_ok(fn, h_radius, n_labels) || !radii_ok(fn, h_radius, n_labels)) return SGPR_E_INVALID;
    if (!not_negative(fn, "tau_z", tau_z)) return SGPR_E_INVALID;
    if (!session_table_ok(fn.c_str(), "", h_starts, n_sessions, Q)) return SGPR_E_INVALID;
    if ((long long)session_base + (n_sessions > 0 ? n_sessions : 1) > 64) {
        set_error(fn + ": session_base " + std::to_string(session_base) + " + " + std::to_string(n_sessions > 0 ? n_sessions : 1) +
                  " sessions exceed the 64 bits of a session mask");
        return SGPR_E_INVALID;
    }
    const long long nodes = (long long)Q * (long long)N;
    if (nodes > (1ll << 30) || (long long)node_base + nodes > 0x7fffffffll) {
        set_error(fn + ": Q N = " + std::to_string(nodes) + " with node_base " + std::to_string(node_base) +
                  " exceeds the int32 node index (Q N <= 2^30)");
        return SGPR_E_INVALID;
    }
    if (Q == 0 || N == 0) return SGPR_OK;
    const bool outs = d_out_center && d_out_label && d_out_count && d_out_first && d_out_sessions && d_out_spread;
    const bool ins = d_lm_center && d_lm_label && d_lm_count && d_lm_first && d_lm_sessions && d_lm_spread;
    if (!d_centers || !d_labels || !d_poses || !d_assoc || (!outs && max_landmarks > 0) || (!ins && L > 0) || !d_node_landmark ||
        !d_num || !d_workspace) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t P = (size_t)nodes, Ls = (size_t)L;
    const size_t need = upd_ws_bytes(P, Ls);
    if (!workspace_ok(fn, workspace_bytes, need)) return SGPR_E_INVALID;

    unsigned char* base = static_cast<unsigned char*>(d_workspace);
    Carver ws{base + lm_core_workspace_bytes(P)};                // (the core's part comes first)
    UpdWs w;
    w.mlab = ws.take<int>(P);
    w.obs = ws.take<int>(P);
    w.sum = ws.take<long long>(3 * Ls);
    w.q = ws.take<unsigned long long>(Ls);
    w.sess = ws.take<unsigned long long>(Ls);
    w.cnt = ws.take<int>(Ls);
    w.tally = ws.take<int>(64);
    w.centre = ws.take<double>(3 * Ls);
    w.core_num = ws.take<int>(64);

    UpdArgs a = {};
    a.centers = d_centers;
    a.labels = d_labels;
    a.poses = d_poses;
    a.assoc = d_assoc;
    a.lm_center = d_lm_center;
    a.lm_label = d_lm_label;
    a.lm_count = d_lm_count;
    a.lm_first = d_lm_first;
    a.lm_sessions = reinterpret_cast<const unsigned long long*>(d_lm_sessions);
    a.lm_spread = d_lm_spread;
    a.out_center = d_out_center;
    a.out_label = d_out_label;
    a.out_count = d_out_count;
    a.out_first = d_out_first;
    a.out_sessions = reinterpret_cast<unsigned long long*>(d_out_sessions);
    a.out_spread = d_out_spread;
    a.node_landmark = d_node_landmark;
    a.num = d_num;
    a.P = (int)P;
    a.N = N;
    a.L = L;
    a.n_labels = n_labels;
    a.session_base = session_base;
    for (int l = 0; l < n_labels; ++l) a.radius[l] = h_radius[l];
    fill_session_table(a.starts, &a.n_sessions, h_starts, n_sessions);

    LmCoreJob job = {};
    job.centers = d_centers;
    job.labels = w.mlab;
    job.poses = d_poses;
    job.G = Q;
    job.N = N;
    job.h_starts = h_starts;
    job.n_sessions = n_sessions;
    job.h_radius = h_radius;
    job.n_labels = n_labels;
    job.tau_z = tau_z;
    job.id_base = L;
    job.first_base = node_base;
    job.session_shift = session_base;
    job.max_landmarks = max_landmarks;
    job.lm_center = d_out_center;
    job.lm_label = d_out_label;
    job.lm_count = d_out_count;
    job.lm_first = d_out_first;
    job.lm_sessions = d_out_sessions;
    job.lm_spread = d_out_spread;
    job.node_landmark = d_node_landmark;
    job.num = w.core_num;

    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(w.sum, 0, upd_zero_bytes(Ls), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_update: memset");
    const dim3 nodes_grid((unsigned)((P + LM_THREADS - 1) / LM_THREADS)), lm_grid((unsigned)((Ls + LM_THREADS - 1) / LM_THREADS)),
        block(LM_THREADS);
    hipLaunchKernelGGL(upd_classify_kernel, nodes_grid, block, 0, s, w, a);
    if (L > 0) {
        hipLaunchKernelGGL(upd_centre_kernel, lm_grid, block, 0, s, w, a);
        hipLaunchKernelGGL(upd_spread_kernel, nodes_grid, block, 0, s, w, a);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_update: launch");
    const int rc = lm_core_launch("sgpr_landmark_update", job, d_workspace, s);
    if (rc != SGPR_OK) return rc;
    hipLaunchKernelGGL(upd_finish_kernel, dim3(L > 0 ? lm_grid.x : 1u), block, 0, s, w, a);
    if (L > 0) hipLaunchKernelGGL(upd_merge_kernel, nodes_grid, block, 0, s, w, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_update: launch");
    return SGPR_OK;
}

}  // extern "C"
