// Track drives through a landmark map (sgpr_landmark_track; include/sgpr_landmark_track.h): the scans of
// a track in order, each predicted from the aligned pose of its predecessor and the odometry between the two, aligned by
// a schedule of gates and accepted or LOST.  Float64 with every operation rounded on its own.  A stage is
// sgpr_landmark_align of one scan, and it is the same code: la_fit_scan of sgpr_landmark_align_core.hpp, which
// la_align_kernel runs too.
//
//   lt_prep_kernel    one thread per landmark and stage: eligible or not under THAT stage's radii, and an eligible
//                     landmark enters that stage's cell table - cells as wide as that stage's radius, which is what the
//                     nine-cell walk of la_match needs - and is pushed on its cell's list.  The workspace holds n_stages
//                     copies of align's table.
//   lt_track_kernel   one wave per track, four per workgroup, serial over the track's scans inside the launch.  The
//                     aligned pose of the previous scan, its odometry pose and whether it was lost live in registers.  A
//                     scan is read about 2 (iters + 1) n_stages times: when N <= LT_LDS_SLOTS the wave copies its
//                     (x, y, z, label) into its own quarter of the LDS once per scan - lane j stages and reads the slots
//                     j, j + 64, .., its own, so no barrier is needed - and any larger N reads global memory through the
//                     accessor align uses.  No wave waits for another: nothing here can deadlock.  Lane 0 writes the
//                     scan's outputs; the four counts of d_num are integer atomics at the end of a track.
//
// -DSGPR_ALIGN_SEARCH=2 builds the form that tests every landmark, as in sgpr_landmark_align.hip.  Integer atomics only,
// no inline assembly, plain vector stores.  The argument checks are sgpr_map.hpp's and sgpr_map_grid.hpp's, the stage-
// worded radius message included (radii_ok).
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_align_core.hpp"
#include "sgpr_landmark_track.h"
#include "sgpr_map_grid.hpp"

#ifndef SGPR_ALIGN_SEARCH
#define SGPR_ALIGN_SEARCH 1
#endif

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int LT_THREADS = 256;
constexpr int LT_WAVES = LT_THREADS / 64;
constexpr int LT_LDS_SLOTS = 256;              // slots of a scan a wave can stage: 4 waves x 256 x 16 bytes = 16 KiB
constexpr bool LT_TABLE = SGPR_ALIGN_SEARCH != 2;

struct LtArgs {
    const float* centers;
    const int32_t* labels;
    const double* odom;
    const double* init;
    LaMap m;
    LaTable t[SGPR_TRACK_MAX_STAGES];
    double* poses_out;
    double* pred_out;
    int32_t* node_landmark;
    int32_t* stat;
    double* rms;
    int32_t* num;
    int Q, N, n_tracks, n_stages, n_reacquire, iters, min_nodes, min_matched, flags;
    double max_shift2;                         // max_shift max_shift, formed once
    int32_t starts[SGPR_SESSION_MAX];
    double radius[SGPR_TRACK_MAX_STAGES][SGPR_LANDMARK_MAX_LABELS];
};

__global__ __launch_bounds__(LT_THREADS) void lt_prep_kernel(const LtArgs a) {
    const int i = blockIdx.x * LT_THREADS + threadIdx.x, s = blockIdx.y;
    if (i >= a.m.L) return;
    la_prep_landmark<LT_TABLE>(a.m, a.t[s], a.radius[s], i);
}

// a scan in the wave's LDS: (x, y, z, label) bits per slot
struct LtScanLds {
    const int4* p;
    __device__ __forceinline__ int label(int n) const { return p[n].w; }
    __device__ __forceinline__ double x(int n) const { return (double)__int_as_float(p[n].x); }
    __device__ __forceinline__ double y(int n) const { return (double)__int_as_float(p[n].y); }
    __device__ __forceinline__ double z(int n) const { return (double)__int_as_float(p[n].z); }
};

__device__ __forceinline__ Se2 lt_load(const double* p) { return Se2{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void lt_store(double* p, const Se2& v) {
    p[0] = v.c;
    p[1] = v.s;
    p[2] = v.x;
    p[3] = v.y;
}

template <bool TABLE, bool LDS>
__global__ __launch_bounds__(LT_THREADS) void lt_track_kernel(const LtArgs a) {
    __shared__ int4 staged[LDS ? LT_WAVES * LT_LDS_SLOTS : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * LT_WAVES + wave;
    if (t >= a.n_tracks) return;                                // (whole waves leave: the shuffles are wave-wide)
    const int lo = a.starts[t], hi = t + 1 < a.n_tracks ? a.starts[t + 1] : a.Q;
    if (lo >= hi) return;
    const Se2 init = lt_load(a.init + 4 * (size_t)t);
    const bool init_ok = se2_finite(init);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    int4* mine = staged + (LDS ? wave * LT_LDS_SLOTS : 0);

    Se2 A = init, Oprev = init;
    bool prev_lost = (a.flags & SGPR_TRACK_START_LOST) != 0;
    int tracked = 0, lost_scans = 0, run = 0, longest = 0;
    for (int i = lo; i < hi; ++i) {
        const size_t base = (size_t)i * (size_t)a.N;
        int32_t* row = a.node_landmark + base;
        if (!init_ok) {
            for (int n = lane; n < a.N; n += 64) row[n] = -1;
            if (lane == 0) {
                lt_store(a.poses_out + 4 * (size_t)i, init);
                lt_store(a.pred_out + 4 * (size_t)i, init);
                a.rms[i] = qnan;
                int32_t* st = a.stat + 4 * (size_t)i;
                st[0] = 0;
                st[1] = 0;
                st[2] = 0;
                st[3] = SGPR_TRACK_NONFINITE;
            }
            continue;
        }
        // 1. prediction
        const Se2 O = lt_load(a.odom + 4 * (size_t)i);
        int flags = 0;
        Se2 P = init;
        if (i > lo) {
            if (se2_finite(Oprev) && se2_finite(O)) {
                P = se2_compose(A, se2_compose(se2_inverse(Oprev), O));
            } else {
                P = A;
                flags |= SGPR_TRACK_NO_ODOM;
            }
        }
        Oprev = O;
        // 2. stages
        const float* cen = a.centers + 3 * base;
        const int32_t* lab = a.labels + base;
        if (LDS)
            for (int n = lane; n < a.N; n += 64)
                mine[n] = make_int4(__float_as_int(cen[3 * (size_t)n]), __float_as_int(cen[3 * (size_t)n + 1]),
                                    __float_as_int(cen[3 * (size_t)n + 2]), lab[n]);
        const bool reacquire = prev_lost && a.n_reacquire > 0;
        if (reacquire) flags |= SGPR_TRACK_REACQUIRE;
        Se2 X = P;
        LaFit f = {0, 0, 0, 0, 0.0};
        int refits = 0;
        for (int s = reacquire ? 0 : a.n_reacquire; s < a.n_stages; ++s) {
            if (LDS) {
                const LtScanLds sc = {mine};
                f = la_fit_scan<TABLE>(a.m, a.t[s], a.radius[s], sc, a.N, lane, row, a.iters, a.min_nodes, X);
            } else {
                const LaScanGlobal sc = {cen, lab};
                f = la_fit_scan<TABLE>(a.m, a.t[s], a.radius[s], sc, a.N, lane, row, a.iters, a.min_nodes, X);
            }
            refits += f.refits;
            flags |= f.flags;
        }
        const double rms = la_rms(f);
        // 3. accept or reject
        const double dx = X.x - P.x, dy = X.y - P.y;
        const bool lost = f.matched < a.min_matched || dx * dx + dy * dy > a.max_shift2;
        if (lost) flags |= SGPR_TRACK_LOST;
        A = lost ? P : X;
        prev_lost = lost;
        run = lost ? run + 1 : 0;
        longest = run > longest ? run : longest;
        lost_scans += lost ? 1 : 0;
        tracked += (flags & (SGPR_TRACK_LOST | SGPR_TRACK_NONFINITE)) == 0 ? 1 : 0;
        if (lane == 0) {
            lt_store(a.poses_out + 4 * (size_t)i, A);
            lt_store(a.pred_out + 4 * (size_t)i, P);
            a.rms[i] = rms;
            int32_t* st = a.stat + 4 * (size_t)i;
            st[0] = f.matched;
            st[1] = f.live;
            st[2] = refits;
            st[3] = flags;
        }
    }
    if (lane != 0) return;
    if (tracked) atomicAdd(&a.num[0], tracked);
    if (lost_scans) atomicAdd(&a.num[1], lost_scans);
    if (longest) atomicMax(&a.num[2], longest);
    atomicAdd(&a.num[3], 1);
}

bool lt_stages_ok(int n_stages) { return n_stages >= 1 && n_stages <= SGPR_TRACK_MAX_STAGES; }

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_track_workspace_bytes(int Q, int N, int L, int n_stages) {
    if (!la_size_ok(Q, N, L) || !lt_stages_ok(n_stages) || Q == 0 || N == 0) return 0;
    return (size_t)n_stages * la_table_bytes((size_t)L);
}

int sgpr_landmark_track(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_odom,
                        const int32_t* h_starts, int n_tracks, const double* d_init, const double* d_lm_center,
                        const int32_t* d_lm_label, const uint8_t* d_lm_use, int L, const double* h_radius, int n_stages,
                        int n_reacquire, int n_labels, double tau_z, int iters, int min_nodes, int min_matched,
                        double max_shift, int flags, double* d_poses_out, double* d_pred_out, int32_t* d_node_landmark,
                        int32_t* d_stat, double* d_rms, int32_t* d_num, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
    const std::string fn = "sgpr_landmark_track";
    if (!no_negative(fn, {{"Q", Q}, {"N", N}, {"L", L}, {"iters", iters}})) return SGPR_E_INVALID;
    if (!lt_stages_ok(n_stages)) {
        set_error(fn + ": n_stages " + std::to_string(n_stages) + " outside [1, " + std::to_string(SGPR_TRACK_MAX_STAGES) + "]");
        return SGPR_E_INVALID;
    }
    if (n_reacquire < 0 || n_reacquire >= n_stages) {
        set_error(fn + ": n_reacquire " + std::to_string(n_reacquire) + " outside [0, n_stages - 1]");
        return SGPR_E_INVALID;
    }
    if (min_nodes < 2) {
        set_error(fn + ": min_nodes " + std::to_string(min_nodes) + " is below 2");
        return SGPR_E_INVALID;
    }
    if (min_matched < 0) {
        set_error(fn + ": min_matched " + std::to_string(min_matched) + " is negative");
        return SGPR_E_INVALID;
    }
    if (!landmark_labels_ok(fn, h_radius, n_labels)) return SGPR_E_INVALID;
    for (int j = 0; j < n_stages; ++j)
        if (!radii_ok(fn, h_radius + (size_t)j * n_labels, n_labels, "radius", j)) return SGPR_E_INVALID;
    if (!not_negative(fn, "tau_z", tau_z)) return SGPR_E_INVALID;
    if (!not_negative(fn, "max_shift", max_shift)) return SGPR_E_INVALID;
    if (!session_table_ok(fn.c_str(), "track", h_starts, n_tracks, Q)) return SGPR_E_INVALID;
    if (!la_size_ok(Q, N, L)) {
        set_error(fn + ": Q N = " + std::to_string((long long)Q * N) + " exceeds the int32 node index");
        return SGPR_E_INVALID;
    }
    if (Q == 0 || N == 0) return SGPR_OK;
    if (!d_centers || !d_labels || !d_odom || !d_init || ((!d_lm_center || !d_lm_label) && L > 0) || !d_poses_out || !d_pred_out ||
        !d_node_landmark || !d_stat || !d_rms || !d_num || !d_workspace) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = (size_t)n_stages * la_table_bytes((size_t)L);
    if (!workspace_ok(fn, workspace_bytes, need)) return SGPR_E_INVALID;

    Carver ws{static_cast<unsigned char*>(d_workspace)};
    LtArgs a = {};
    a.centers = d_centers;
    a.labels = d_labels;
    a.odom = d_odom;
    a.init = d_init;
    a.m = LaMap{d_lm_center, d_lm_label, d_lm_use, L, n_labels, tau_z};
    for (int j = 0; j < n_stages; ++j) a.t[j] = la_table_carve(ws, (size_t)L);
    a.poses_out = d_poses_out;
    a.pred_out = d_pred_out;
    a.node_landmark = d_node_landmark;
    a.stat = d_stat;
    a.rms = d_rms;
    a.num = d_num;
    a.Q = Q;
    a.N = N;
    a.n_stages = n_stages;
    a.n_reacquire = n_reacquire;
    a.iters = iters;
    a.min_nodes = min_nodes;
    a.min_matched = min_matched;
    a.flags = flags;
    a.max_shift2 = max_shift * max_shift;
    fill_session_table(a.starts, &a.n_tracks, h_starts, n_tracks);
    for (int j = 0; j < n_stages; ++j)
        for (int l = 0; l < n_labels; ++l) a.radius[j][l] = h_radius[(size_t)j * n_labels + l];

    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(d_num, 0, 4 * sizeof(int32_t), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_track: memset");
    if (LT_TABLE)
        for (int j = 0; j < n_stages; ++j) {
            // cell_key | cell_head of stage j: empty keys, list ends (-1)
            e = hipMemsetAsync(a.t[j].g.cell_key, 0xff, grid_clear_bytes((size_t)L), s);
            if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_track: memset");
        }
    const dim3 block(LT_THREADS), track_grid((a.n_tracks + LT_WAVES - 1) / LT_WAVES);
    if (L > 0) hipLaunchKernelGGL(lt_prep_kernel, dim3((L + LT_THREADS - 1) / LT_THREADS, n_stages), block, 0, s, a);
    if (N <= LT_LDS_SLOTS)
        hipLaunchKernelGGL((lt_track_kernel<LT_TABLE, true>), track_grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((lt_track_kernel<LT_TABLE, false>), track_grid, block, 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_track: launch");
    return SGPR_OK;
}

}  // extern "C"
