// Joining and compacting landmark maps on their records alone (sgpr_landmark_merge; include/sgpr_landmark_merge.h,
// DESIGN.md §36): the records of map A and, moved by one planar pose, of map B are input points; what a keep mask or the
// eligible rule drops is gone, records of one label within the label's radius link, and every connected component
// becomes one record, as if the observations behind its members had been fused.  §27's sequence on records instead of
// nodes: HBM-bound integer / pointer work, no matrix cores.
//
//   mrg_prepare_kernel    one thread per input record t (A: t < L_a, B: L_a + j): the INPUT RECORD (B's centre under the
//                         pose), kept or not, eligible or not.  An eligible record enters the open-addressing cell table
//                         (key: a hash of (label, ix, iy)) and is pushed on its cell's list.  Every thread initialises its
//                         own slot of the forest and of the accumulators.  The two kinds of dropped records are counted
//                         per wave, one atomic each.
//   mrg_union_kernel      one thread per eligible record: the lower-indexed records on the lists of its 9 neighbouring
//                         cells are tested with the header's rule and united; the larger root is hooked under the smaller,
//                         so a component's root is its LOWEST INPUT INDEX whatever the execution order.
//   mrg_flatten_kernel    the forest is final: every eligible record finds its root and adds - ONCE, here, not where a
//                         list is walked - its count, its member, its three fixed-point weighted coordinates, its
//                         sessions (atomicOr) and its first (atomicMin) to the root.  Each workgroup counts its roots.
//   mrg_scan_kernel       one workgroup: exclusive prefix sum of the per-workgroup root counts; L'.
//   mrg_record_kernel     the id of a root = the roots before it; the centre of a fused component goes to the workspace;
//                         records of ids below max_out are written - the input record of a component of one - and the
//                         fused components are counted.
//   mrg_spread_kernel     one thread per input record: d_old_to_new; a member of a fused component adds its
//                         parallel-axis term about the new centre to Q of its root.
//   mrg_finish_kernel     spread of every fused record below max_out; one thread fills d_num.
//
// The cell table and the union-find are sgpr_map.hpp's, with their SIZING, VISIBILITY and TERMINATION arguments: the
// table has table_slots(L_a + L_b) slots and every key in it belongs to some record; the lists are complete before the
// kernel that walks them starts; the forest is the only memory another workgroup rewrites while it is read.  Every loop
// is bounded by a list's length or the forest's depth, and no wave waits for another workgroup.  The push on a cell's
// list, the linking step of mrg_union_kernel, the count, the scan and the rank of the numbering and the eligible rule are
// sgpr_map_grid.hpp's (grid_push, link_item, block_count, scan_block_counts, rank_in_block, record_eligible).
//
// CELLS.  An eligible centre obeys |p_k| <= |p_k n| <= 2^38, one bit more than the 2^37 of sgpr_map.hpp's proof that two
// points in range are never two cells apart: the two rounded quotients then err by 2^-14 each, 1.3e-4 together, still
// below the 9e-4 the cell width leaves, and |quotient| <= 2^39 fits a long long.
//
// CONTENTION.  The atomics on one root's accumulators are bounded by the records that fuse into one landmark - a few;
// there is no per-wave pre-reduction (the all-on-one case is tested for its bits, not tuned).
//
// One memset fills the table (empty keys, list ends), one zeroes the counters; nothing else of the workspace is read
// before it is written.  No floating-point atomics, no inline assembly, plain vector stores.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_merge.h"
#include "sgpr_map_grid.hpp"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int MRG_THREADS = NUMBER_THREADS;
constexpr long long MRG_COUNT_TOP = 0x7fffffffll;

struct MrgWs {
    double* p;                     // [T][3] centre of the input record
    long long* sum;                // [T][3] fixed-point weighted coordinate sums per root
    double* centre;                // [T][3] center' of a fused root
    unsigned long long* cnt;       // [T] sum of the counts per root
    unsigned long long* q;         // [T] Q' per root
    unsigned long long* sess;      // [T] sessions per root
    int* lab;                      // [T] label of an eligible record, -1 of a dropped one
    int* parent;                   // [T] union-find forest
    int* next;                     // [T] list of the record's cell; after flatten: the record's root
    int* members;                  // [T] members per root
    int* first;                    // [T] lowest first per root
    int* id;                       // [T] output id of a root
    unsigned long long* cell_key;  // [H]
    int* cell_head;                // [H]
    int* blk_roots;                // [B] roots per workgroup; after the scan: roots before the workgroup
    int* tally;                    // [64] (dropped by a mask, dropped as ineligible, fused components, L')
    unsigned long long hmask;      // H - 1 (H a power of two)
    // (next, cell_key, cell_head, hmask) as the grid the shared steps take
    __device__ __forceinline__ CellGrid grid() const { return CellGrid{next, cell_key, cell_head, hmask}; }
};

struct MrgMap {
    const double* center;
    const int32_t* label;
    const int32_t* count;
    const int32_t* first;
    const unsigned long long* sessions;
    const double* spread;
    const uint8_t* keep;
};

struct MrgArgs {
    MrgMap a, b;
    double* out_center;
    int32_t* out_label;
    int32_t* out_count;
    int32_t* out_first;
    unsigned long long* out_sessions;
    double* out_spread;
    int32_t* old_to_new;
    int32_t* num;
    int T, L_a, n_labels, max_out, B;
    int has_pose, session_shift, first_base;
    double tau_z;
    double pose[4];
    double radius[SGPR_LANDMARK_MAX_LABELS];
};

// what of the INPUT RECORD is not its centre (the centre is in the workspace: MrgWs::p)
struct MrgRest {
    int label, count, first;
    unsigned long long sessions;
    double spread;
};

__device__ __forceinline__ MrgRest mrg_rest(const MrgArgs& a, int t) {
    const bool in_b = t >= a.L_a;
    const MrgMap& m = in_b ? a.b : a.a;
    const int i = in_b ? t - a.L_a : t;
    MrgRest r;
    r.label = m.label[i];
    r.count = m.count[i];
    r.spread = m.spread[i];
    const int f = m.first[i];
    const unsigned long long s = m.sessions[i];
    r.first = in_b ? (int)((unsigned)f + (unsigned)a.first_base) : f;
    r.sessions = in_b ? s << a.session_shift : s;
    return r;
}

__global__ __launch_bounds__(MRG_THREADS) void mrg_prepare_kernel(const MrgWs w, const MrgArgs a) {
    const int t = blockIdx.x * MRG_THREADS + threadIdx.x;
    bool masked = false, unfit = false;
    if (t < a.T) {
        const bool in_b = t >= a.L_a;
        const MrgMap& m = in_b ? a.b : a.a;
        const int i = in_b ? t - a.L_a : t;
        double px = m.center[3 * (size_t)i], py = m.center[3 * (size_t)i + 1];
        const double pz = m.center[3 * (size_t)i + 2];
        if (in_b && a.has_pose) se2_apply(Se2{a.pose[0], a.pose[1], a.pose[2], a.pose[3]}, px, py, &px, &py);
        w.p[3 * (size_t)t] = px;
        w.p[3 * (size_t)t + 1] = py;
        w.p[3 * (size_t)t + 2] = pz;
        const int l = m.label[i], n = m.count[i];
        const bool kept = !m.keep || m.keep[i] != 0;
        const bool ok = record_eligible(l, n, m.spread[i], px, py, pz, a.radius, a.n_labels);
        masked = !kept;
        unfit = kept && !ok;
        const bool live = kept && ok;
        w.lab[t] = live ? l : -1;
        w.parent[t] = t;
        w.members[t] = 0;
        w.first[t] = 0x7fffffff;
        w.id[t] = -1;
        w.cnt[t] = 0ull;
        w.q[t] = 0ull;
        w.sess[t] = 0ull;
        w.sum[3 * (size_t)t] = 0;
        w.sum[3 * (size_t)t + 1] = 0;
        w.sum[3 * (size_t)t + 2] = 0;
        if (live) grid_push(w.grid(), t, l, lm_cell_width(a.radius[l]), px, py);
        else w.next[t] = -1;
    }
    const unsigned long long masks = __ballot(masked), unfits = __ballot(unfit);
    if ((threadIdx.x & 63) == 0) {
        if (masks) atomicAdd(&w.tally[0], __popcll(masks));
        if (unfits) atomicAdd(&w.tally[1], __popcll(unfits));
    }
}

__global__ __launch_bounds__(MRG_THREADS) void mrg_union_kernel(const MrgWs w, const MrgArgs a) {
    const int t = blockIdx.x * MRG_THREADS + threadIdx.x;
    if (t >= a.T) return;
    link_item(w.grid(), w.p, w.lab, w.parent, a.radius, a.tau_z, t);
}

__global__ __launch_bounds__(MRG_THREADS) void mrg_flatten_kernel(const MrgWs w, const MrgArgs a) {
    __shared__ int wsum[MRG_THREADS / 64];
    const int t = blockIdx.x * MRG_THREADS + threadIdx.x;
    const bool live = t < a.T && w.lab[t] >= 0;
    int root = -1;
    if (live) {
        root = uf_root_final(w.parent, t);
        w.next[t] = root;                                       // (the cell lists are dead) the record's root
        const MrgRest rec = mrg_rest(a, t);
        const double n = (double)rec.count;
        atomicAdd(&w.cnt[root], (unsigned long long)rec.count);
        atomicAdd(&w.members[root], 1);
        for (int k = 0; k < 3; ++k)
            atomicAdd(reinterpret_cast<unsigned long long*>(&w.sum[3 * (size_t)root + k]),
                      (unsigned long long)llrint((w.p[3 * (size_t)t + k] * n) * MAP_FIX));
        atomicOr(&w.sess[root], rec.sessions);
        atomicMin(&w.first[root], rec.first);
    }
    const int roots = block_count(live && root == t, wsum);
    if (threadIdx.x == 0) w.blk_roots[blockIdx.x] = roots;
}

__global__ __launch_bounds__(SCAN_THREADS) void mrg_scan_kernel(const MrgWs w, const MrgArgs a) {
    __shared__ int part[SCAN_THREADS];
    scan_block_counts<false>(w.blk_roots, nullptr, a.B, part, nullptr);
    if (threadIdx.x == SCAN_THREADS - 1) w.tally[3] = part[threadIdx.x];
}

__global__ __launch_bounds__(MRG_THREADS) void mrg_record_kernel(const MrgWs w, const MrgArgs a) {
    __shared__ int wcount[MRG_THREADS / 64];
    const int t = blockIdx.x * MRG_THREADS + threadIdx.x;
    const bool root = t < a.T && w.lab[t] >= 0 && w.next[t] == t;
    const int members = root ? w.members[t] : 0;
    const unsigned long long fused = __ballot(members > 1);
    if ((threadIdx.x & 63) == 0 && fused) atomicAdd(&w.tally[2], __popcll(fused));
    const int rank = rank_in_block(root, wcount);
    if (!root) return;
    const int id = w.blk_roots[blockIdx.x] + rank;
    w.id[t] = id;
    double c[3];
    if (members > 1) {
        const double cnt = (double)(long long)w.cnt[t];
        for (int k = 0; k < 3; ++k) {
            c[k] = (double)w.sum[3 * (size_t)t + k] / (cnt * MAP_FIX);
            w.centre[3 * (size_t)t + k] = c[k];
        }
    } else {
        for (int k = 0; k < 3; ++k) c[k] = w.p[3 * (size_t)t + k];
    }
    if (id >= a.max_out) return;
    const MrgRest rec = mrg_rest(a, t);
    for (int k = 0; k < 3; ++k) a.out_center[3 * (size_t)id + k] = c[k];
    a.out_label[id] = rec.label;
    if (members > 1) {
        const long long sum = (long long)w.cnt[t];
        a.out_count[id] = (int)(sum < MRG_COUNT_TOP ? sum : MRG_COUNT_TOP);
        a.out_first[id] = w.first[t];
        a.out_sessions[id] = w.sess[t];
    } else {
        a.out_count[id] = rec.count;
        a.out_first[id] = rec.first;
        a.out_sessions[id] = rec.sessions;
        a.out_spread[id] = rec.spread;
    }
}

__global__ __launch_bounds__(MRG_THREADS) void mrg_spread_kernel(const MrgWs w, const MrgArgs a) {
    const int t = blockIdx.x * MRG_THREADS + threadIdx.x;
    if (t >= a.T) return;
    if (w.lab[t] < 0) {
        a.old_to_new[t] = -1;
        return;
    }
    const int root = w.next[t];
    a.old_to_new[t] = w.id[root];
    if (w.members[root] < 2) return;
    const MrgRest rec = mrg_rest(a, t);
    const double ax = w.p[3 * (size_t)t] - w.centre[3 * (size_t)root], ay = w.p[3 * (size_t)t + 1] - w.centre[3 * (size_t)root + 1];
    const double v = rec.spread * rec.spread + (ax * ax + ay * ay);
    atomicAdd(&w.q[root], (unsigned long long)llrint((fmin(v, MAP_D2_CAP) * (double)rec.count) * MAP_FIX));
}

__global__ __launch_bounds__(MRG_THREADS) void mrg_finish_kernel(const MrgWs w, const MrgArgs a) {
    const int t = blockIdx.x * MRG_THREADS + threadIdx.x;
    if (t == 0) {
        a.num[0] = w.tally[3];
        a.num[1] = w.tally[0];
        a.num[2] = w.tally[1];
        a.num[3] = w.tally[2];
    }
    if (t >= a.T || w.lab[t] < 0 || w.next[t] != t || w.members[t] < 2) return;
    const int id = w.id[t];
    if (id >= a.max_out) return;
    a.out_spread[id] = sqrt((double)w.q[t] / ((double)(long long)w.cnt[t] * MAP_FIX));
}

bool mrg_size_ok(int L_a, int L_b) { return L_a >= 0 && L_b >= 0 && (long long)L_a + (long long)L_b <= 0x7fffffffll; }

size_t mrg_ws_bytes(size_t T) {
    const size_t b = (T + MRG_THREADS - 1) / MRG_THREADS;
    return align256(T * 24) * 3 + align256(T * 8) * 3 + align256(T * 4) * 5 + grid_bytes(T) + align256(b * 4) + align256(64 * 4);
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_merge_workspace_bytes(int L_a, int L_b) {
    if (!mrg_size_ok(L_a, L_b) || (long long)L_a + L_b == 0) return 0;
    return mrg_ws_bytes((size_t)L_a + (size_t)L_b);
}

int sgpr_landmark_merge(const double* d_a_center, const int32_t* d_a_label, const int32_t* d_a_count,
                        const int32_t* d_a_first, const uint64_t* d_a_sessions, const double* d_a_spread,
                        const uint8_t* d_keep_a, int L_a, const double* d_b_center, const int32_t* d_b_label,
                        const int32_t* d_b_count, const int32_t* d_b_first, const uint64_t* d_b_sessions,
                        const double* d_b_spread, const uint8_t* d_keep_b, int L_b, const double* h_pose,
                        int session_shift, int first_base, const double* h_radius, int n_labels, double tau_z,
                        int max_out, double* d_out_center, int32_t* d_out_label, int32_t* d_out_count,
                        int32_t* d_out_first, uint64_t* d_out_sessions, double* d_out_spread, int32_t* d_old_to_new,
                        int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_merge";
    if (!no_negative(fn, {{"L_a", L_a}, {"L_b", L_b}, {"max_out", max_out}, {"first_base", first_base}})) return SGPR_E_INVALID;
    if (!mrg_size_ok(L_a, L_b)) {
        set_error(fn + ": L_a + L_b = " + std::to_string((long long)L_a + L_b) + " exceeds the int32 record index");
        return SGPR_E_INVALID;
    }
    if (session_shift < 0 || session_shift > 63) {
        set_error(fn + ": session_shift " + std::to_string(session_shift) + " outside [0, 63]");
        return SGPR_E_INVALID;
    }
    if (!landmark_labels_ok(fn, h_radius, n_labels) || !radii_ok(fn, h_radius, n_labels)) return SGPR_E_INVALID;
    if (!not_negative(fn, "tau_z", tau_z)) return SGPR_E_INVALID;
    if (h_pose)
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(h_pose[k])) {
                set_error(fn + ": h_pose[" + std::to_string(k) + "] is not finite");
                return SGPR_E_INVALID;
            }
    const size_t T = (size_t)L_a + (size_t)L_b;
    if (T == 0) return SGPR_OK;
    const bool in_a = d_a_center && d_a_label && d_a_count && d_a_first && d_a_sessions && d_a_spread;
    const bool in_b = d_b_center && d_b_label && d_b_count && d_b_first && d_b_sessions && d_b_spread;
    const bool outs = d_out_center && d_out_label && d_out_count && d_out_first && d_out_sessions && d_out_spread;
    if ((!in_a && L_a > 0) || (!in_b && L_b > 0) || (!outs && max_out > 0) || !d_old_to_new || !d_num || !d_workspace) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    if (!workspace_ok(fn, workspace_bytes, mrg_ws_bytes(T))) return SGPR_E_INVALID;

    const size_t H = table_slots(T);
    const int B = (int)((T + MRG_THREADS - 1) / MRG_THREADS);
    Carver ws{static_cast<unsigned char*>(d_workspace)};
    MrgWs w;
    w.hmask = H - 1;
    w.p = ws.take<double>(3 * T);
    w.sum = ws.take<long long>(3 * T);
    w.centre = ws.take<double>(3 * T);
    w.cnt = ws.take<unsigned long long>(T);
    w.q = ws.take<unsigned long long>(T);
    w.sess = ws.take<unsigned long long>(T);
    w.lab = ws.take<int>(T);
    w.parent = ws.take<int>(T);
    w.next = ws.take<int>(T);
    w.members = ws.take<int>(T);
    w.first = ws.take<int>(T);
    w.id = ws.take<int>(T);
    w.cell_key = ws.take<unsigned long long>(H);
    w.cell_head = ws.take<int>(H);
    w.blk_roots = ws.take<int>((size_t)B);
    w.tally = ws.take<int>(64);

    MrgArgs a = {};
    a.a = MrgMap{d_a_center, d_a_label, d_a_count, d_a_first, reinterpret_cast<const unsigned long long*>(d_a_sessions), d_a_spread,
                 d_keep_a};
    a.b = MrgMap{d_b_center, d_b_label, d_b_count, d_b_first, reinterpret_cast<const unsigned long long*>(d_b_sessions), d_b_spread,
                 d_keep_b};
    a.out_center = d_out_center;
    a.out_label = d_out_label;
    a.out_count = d_out_count;
    a.out_first = d_out_first;
    a.out_sessions = reinterpret_cast<unsigned long long*>(d_out_sessions);
    a.out_spread = d_out_spread;
    a.old_to_new = d_old_to_new;
    a.num = d_num;
    a.T = (int)T;
    a.L_a = L_a;
    a.n_labels = n_labels;
    a.max_out = max_out;
    a.B = B;
    a.has_pose = h_pose ? 1 : 0;
    a.session_shift = session_shift;
    a.first_base = first_base;
    a.tau_z = tau_z;
    for (int k = 0; k < 4; ++k) a.pose[k] = h_pose ? h_pose[k] : 0.0;
    for (int l = 0; l < n_labels; ++l) a.radius[l] = h_radius[l];

    const hipStream_t s = static_cast<hipStream_t>(stream);
    // cell_key | cell_head: empty keys, list ends (-1)
    hipError_t e = hipMemsetAsync(w.cell_key, 0xff, grid_clear_bytes(T), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.tally, 0, 64 * 4, s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_merge: memset");
    const dim3 grid(B), block(MRG_THREADS);
    hipLaunchKernelGGL(mrg_prepare_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(mrg_union_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(mrg_flatten_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(mrg_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, w, a);
    hipLaunchKernelGGL(mrg_record_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(mrg_spread_kernel, grid, block, 0, s, w, a);
    hipLaunchKernelGGL(mrg_finish_kernel, grid, block, 0, s, w, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_merge: launch");
    return SGPR_OK;
}

}  // extern "C"
