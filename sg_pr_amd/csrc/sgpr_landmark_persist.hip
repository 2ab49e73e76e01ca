// Visibility tallies of a landmark map (sgpr_landmark_persist; include/sgpr_landmark_persist.h): per
// landmark, the scans of a drive that should have seen it and the scans that did, and a mask of the landmarks the drive
// should have seen and did not.  Float64 with every operation rounded on its own; every tally is an integer, so the
// atomics below decide nothing.
//
//   lp_prep_kernel    one thread per landmark: eligible or not - its label, or -1, into the workspace - its two tallies
//                     zeroed, and an eligible landmark enters the COARSE cell table (lp_cell_width: its planar cell only,
//                     no label) and is counted in its cell.  Thread 0 zeroes d_num.
//   lp_offsets_kernel one thread per table slot: a used cell takes its range of the item array from one counter.  The
//                     order of the ranges is whatever the atomics make it; a range is contiguous, and that is all the walk
//                     needs.
//   lp_fill_kernel    one thread per landmark: an eligible landmark takes a place in its cell's range.  Afterwards the
//                     landmarks of a cell are item[pos .. pos + cnt).
//   lp_tally_kernel   one wave per scan, four per workgroup.  Pass A: the live rule, far2 by a wave maximum, v.  Pass B,
//                     owners: a live observing node owns (q, l) when no lower slot of the scan observes l; an owner adds 1
//                     to seen[l], and to expected[l] too when l is not in view.  Pass C: the cells that can hold a
//                     landmark within v - the lanes look them up side by side; a lane walks the items of its own cell when
//                     they are few (at a 50 m view a cell holds four), a fuller cell goes round the wave with the lanes
//                     over its items - and 1 to expected[l] for every landmark in view.  The per-scan counts are wave
//                     sums of integers.
//   lp_decide_kernel  one thread per landmark: d_keep, and the three landmark counters of d_num by one atomic per wave.
//
// TWO SEARCHES, the same bits.  SGPR_PERSIST_SEARCH == 2, the build's: pass C tests every landmark, the lanes over the
// landmarks; lp_offsets_kernel, lp_fill_kernel and the memsets are not launched.  It is the build's because it was the
// faster at both sizes measured (114 and 2958 landmarks): the call is bound by its launches, three
// against seven.  -DSGPR_PERSIST_SEARCH=1 builds the cell table described above, whose work per scan does not grow with
// the map.  Its compact layout is there because a linked list per cell, the form of sgpr_landmark_align.hip, gives a
// list to ONE lane, and with max_range = +inf one cell holds every landmark.  Two memsets instead of one: the table's
// empty key is all ones (sgpr_map.hpp), the cell counts start at zero.  The workspace is the same for both.
// No floating-point atomics, no inline assembly, plain vector stores; no workgroup waits for another.
// The 2^37 limit, the map point, the wave sum and the slot of a cell are sgpr_map_grid.hpp's (in_limit37, se2_apply,
// wave_sum, grid_cell_slot); the rectangular walk of pass C visits another neighbourhood than grid_near's and stays here.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_persist.h"
#include "sgpr_map_grid.hpp"

#ifndef SGPR_PERSIST_SEARCH
#define SGPR_PERSIST_SEARCH 2
#endif

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr double LP_CELL_CLAMP = 549755813888.0;   // 2^39: past every cell coordinate of a landmark
constexpr double LP_MIN_PAD = 1e-100;
constexpr int LP_OWNER_STEP = 8;     // lower slots looked at between two looks at the answer (pass B)
constexpr int LP_LANE_ITEMS = 16;    // a cell of up to this many landmarks is walked by one lane (pass C)
constexpr bool LP_TABLE = SGPR_PERSIST_SEARCH != 2;
enum { LP_NONFINITE = 1 };

struct LpArgs {
    const float* centers;
    const int32_t* labels;
    const double* poses;
    const int32_t* assoc;
    const double* lm_center;
    const int32_t* lm_label;
    const unsigned char* lm_use;
    int32_t* expected;
    int32_t* seen;
    unsigned char* keep;
    int32_t* scan_stat;
    double* view;
    int32_t* num;
    int* elab;                     // [L] label of an eligible landmark, -1 of any other
    unsigned* lslot;               // [L] the table slot of an eligible landmark's cell
    int* item;                     // [L] the eligible landmarks, cell by cell
    unsigned long long* cell_key;  // [H]
    int* cell_cnt;                 // [H] landmarks of the cell
    int* cell_pos;                 // [H] first item of the cell (after lp_fill_kernel)
    int* total;                    // items handed out
    unsigned long long hmask;      // H - 1 (H a power of two, at most 2^32: a slot fits lslot)
    int Q, N, L, n_labels, min_expected;
    double max_range, margin, ratio, cell_w;
    double radius[SGPR_LANDMARK_MAX_LABELS];
};

// Width of a coarse cell, from the largest view range any scan of the call can have: vcap = max_range - margin >= v_q
// (min(max_range, .) <= max_range and a difference is rounded monotonically).  Half of it, and never below LM_MIN_CELL:
// v_q <= 2 w for every scan.  A cell as wide as a link radius (sgpr_map.hpp) would put thousands under a 50 m view.
//
// EVERY LANDMARK IN VIEW LIES IN THE CELLS WALKED.  The cell of a coordinate a is floor(fl(a / w)) (lm_cell_coord); fl,
// division by w > 0 and floor are monotone, so a <= b as doubles gives cell(a) <= cell(b) with no error term at all.
// Let the landmark be in view: fl(dx dx + dy dy) <= fl(v v), dx = fl(cx - X).  Then fl(dx dx) <= fl(v v).  Where both
// squares are normal numbers this gives |dx| <= v (1 + 2^-51); where fl(v v) is below 1e-280 it gives |dx| < 1e-139.
// The walk pads v to t = max(fl(1.001 v), 1e-100), above both bounds, so |dx| < t strictly.  Had cx - X >= t in the reals,
// rounding (monotone, t a double) would give dx >= t; so cx - X < t, cx < X + t, and cx = fl(cx) <= fl(X + t).  By the
// monotone chain cell(cx) <= cell(fl(X + t)) = hi; in the same way cell(cx) >= cell(fl(X - t)) = lo; and the same in y.
// The walk covers [lo, hi] in both coordinates, clamped to +-2^39, which no landmark's cell exceeds (|cx| <= 2^37,
// w >= 0.5).  Where X +- t overflows, |X| > 1e308 - t and t < 1e39: no centre within 2^37 is in view and nothing is walked.
//
// THE WALK IS SHORT.  Unclamped ends mean |X +- t| < 2^39 w, so the roundings of the two sums and the two quotients
// add less than 2^-11 to (hi' - lo') = 2 t / w <= 4.005; hi - lo <= 5, at most 6 cells a coordinate and 36 in all.  A clamp
// only shortens the range.  w = +inf (max_range = +inf): every quotient is +-0, one cell.  The hash of two cells may
// collide (lm_cell_key); the walk takes a landmark only from the cell it computes for it, so none is counted twice.
inline double lp_cell_width(double max_range, double margin) {
    const double vcap = max_range - margin;
    return fmax(vcap * 0.5, LM_MIN_CELL);
}

__device__ __forceinline__ double lp_clamped_cell(double v, double w) {
#pragma clang fp contract(off)
    return fmin(fmax(floor(v / w), -LP_CELL_CLAMP), LP_CELL_CLAMP);
}

__global__ __launch_bounds__(LP_THREADS) void lp_prep_kernel(const LpArgs a) {
    const int i = blockIdx.x * LP_THREADS + threadIdx.x;
    if (i == 0) {
        a.num[0] = 0;
        a.num[1] = 0;
        a.num[2] = 0;
        a.num[3] = 0;
    }
    if (i >= a.L) return;
    const int l = a.lm_label[i];
    bool ok = (!a.lm_use || a.lm_use[i] != 0) && l >= 0 && l < a.n_labels;
    const double r = ok ? a.radius[l] : 0.0;
    const double cx = a.lm_center[3 * (size_t)i], cy = a.lm_center[3 * (size_t)i + 1], cz = a.lm_center[3 * (size_t)i + 2];
    ok = ok && r > 0.0 && in_limit37(cx) && in_limit37(cy) && in_limit37(cz);
    a.elab[i] = ok ? l : -1;
    a.expected[i] = 0;
    a.seen[i] = 0;
    if (!ok || !LP_TABLE) return;
    const unsigned long long slot = grid_cell_slot(a.cell_key, a.hmask, 0, a.cell_w, cx, cy);     // (counted, not listed: see above)
    a.lslot[i] = (unsigned)slot;
    atomicAdd(&a.cell_cnt[slot], 1);
}

__global__ __launch_bounds__(LP_THREADS) void lp_offsets_kernel(const LpArgs a) {
    const unsigned long long s = (unsigned long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (s > a.hmask) return;
    const int c = a.cell_cnt[s];
    if (c > 0) a.cell_pos[s] = atomicAdd(a.total, c) + c;       // the END of the range: lp_fill_kernel counts it down
}

__global__ __launch_bounds__(LP_THREADS) void lp_fill_kernel(const LpArgs a) {
    const int i = blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= a.L || a.elab[i] < 0) return;
    a.item[atomicSub(&a.cell_pos[a.lslot[i]], 1) - 1] = i;
}

// the live rule for slot n of a scan under X; x, y: the widened centre in the sensor frame
__device__ __forceinline__ bool lp_live(const LpArgs& a, const Se2& X, bool finite, const float* cen, const int32_t* lab, size_t n,
                                        int& l, double& x, double& y) {
    l = lab[n];
    x = (double)cen[3 * n];
    y = (double)cen[3 * n + 1];
    const double mz = (double)cen[3 * n + 2];
    double mx, my;
    se2_apply(X, x, y, &mx, &my);
    bool alive = finite && l >= 0 && l < a.n_labels;
    const double r = alive ? a.radius[l] : 0.0;
    return alive && r > 0.0 && in_limit37(mx) && in_limit37(my) && in_limit37(mz);
}

// slot n observes landmark id: the node is live and the landmark is eligible and of its label
__device__ __forceinline__ bool lp_observes(const LpArgs& a, const Se2& X, bool finite, const float* cen, const int32_t* lab, size_t n,
                                            int id) {
    int l;
    double x, y;
    return lp_live(a, X, finite, cen, lab, n, l, x, y) && a.elab[id] == l;
}

__device__ __forceinline__ bool lp_in_view(const LpArgs& a, const Se2& X, int id, double v2) {
    const double dx = a.lm_center[3 * (size_t)id] - X.x, dy = a.lm_center[3 * (size_t)id + 1] - X.y;
    return dx * dx + dy * dy <= v2;
}

// pass C on one item of cell (ix, iy): 1, and 1 to expected, when the landmark is of that cell and in view
__device__ __forceinline__ int lp_take(const LpArgs& a, const Se2& X, int id, long long ix, long long iy, double w, double v2) {
    const double cx = a.lm_center[3 * (size_t)id], cy = a.lm_center[3 * (size_t)id + 1];
    if (lm_cell_coord(cx, w) != ix || lm_cell_coord(cy, w) != iy) return 0;      // (a slot two cells share: see lp_cell_width)
    if (!lp_in_view(a, X, id, v2)) return 0;
    atomicAdd(&a.expected[id], 1);
    return 1;
}

template <bool TABLE>
__global__ __launch_bounds__(LP_THREADS) void lp_tally_kernel(const LpArgs a) {
    const int q = blockIdx.x * LP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= a.Q) return;                                       // (whole waves leave: the shuffles below are wave-wide)
    const Se2 X = se2_load(a.poses + 4 * (size_t)q);
    const bool finite = se2_finite(X);
    const size_t N = (size_t)a.N, base = (size_t)q * N;
    const float* cen = a.centers + 3 * base;
    const int32_t* lab = a.labels + base;
    const int32_t* asc = a.assoc + base;

    // pass A: live nodes and the farthest of them in the sensor frame
    double far2 = 0.0;
    int lv = 0;
    for (size_t n = lane; n < N; n += 64) {
        int l;
        double x, y;
        if (!lp_live(a, X, finite, cen, lab, n, l, x, y)) continue;
        lv += 1;
        far2 = fmax(far2, x * x + y * y);
    }
    for (int h = 32; h > 0; h >>= 1) far2 = fmax(far2, __shfl_xor(far2, h));     // (finite and >= 0: a maximum is exact)
    const int live = wave_sum(lv);
    const double v = fmin(a.max_range, sqrt(far2)) - a.margin;
    const bool has_view = v > 0.0;
    const double v2 = v * v;

    // pass B: the owners
    int n_exp = 0, n_seen = 0;
    if (a.L > 0 && live > 0) {
        for (size_t n = lane; n < N; n += 64) {
            const int id = asc[n];
            if (id < 0 || id >= a.L || !lp_observes(a, X, finite, cen, lab, n, id)) continue;
            bool owner = true;
            for (size_t m0 = 0; m0 < n && owner; m0 += LP_OWNER_STEP) {       // (a step's loads are in flight together)
#pragma unroll
                for (int j = 0; j < LP_OWNER_STEP; ++j) {
                    const size_t m = m0 + j < n ? m0 + j : n;                 // (slot n is the node itself: no owner of it)
                    if (m < n && asc[m] == id && lp_observes(a, X, finite, cen, lab, m, id)) owner = false;
                }
            }
            if (!owner) continue;
            n_seen += 1;
            atomicAdd(&a.seen[id], 1);
            if (has_view && lp_in_view(a, X, id, v2)) continue;     // (pass C counts it)
            n_exp += 1;
            atomicAdd(&a.expected[id], 1);
        }
    }

    // pass C: the landmarks in view
    if (a.L > 0 && has_view) {
        if (TABLE) {
            const double t = fmax(v * 1.001, LP_MIN_PAD), w = a.cell_w;
            const double ax = X.x - t, bx = X.x + t, ay = X.y - t, by = X.y + t;
            if (isfinite(ax) && isfinite(bx) && isfinite(ay) && isfinite(by)) {
                const long long lox = (long long)lp_clamped_cell(ax, w), hix = (long long)lp_clamped_cell(bx, w);
                const long long loy = (long long)lp_clamped_cell(ay, w), hiy = (long long)lp_clamped_cell(by, w);
                const long long nx = hix - lox + 1, ncell = nx * (hiy - loy + 1);
                for (long long c0 = 0; c0 < ncell; c0 += 64) {
                    int pos = 0, cnt = 0;
                    if (c0 + lane < ncell) {
                        const unsigned long long s = table_find(a.cell_key, a.hmask, lm_cell_key(0, lox + (c0 + lane) % nx, loy + (c0 + lane) / nx));
                        if (s != TABLE_EMPTY) {
                            pos = a.cell_pos[s];
                            cnt = a.cell_cnt[s];
                        }
                    }
                    // a cell of a few landmarks stays with the lane that found it; a fuller one goes round the wave
                    if (cnt <= LP_LANE_ITEMS) {
                        const long long ix = lox + (c0 + lane) % nx, iy = loy + (c0 + lane) / nx;
                        for (int e = 0; e < cnt; ++e) n_exp += lp_take(a, X, a.item[pos + e], ix, iy, w, v2);
                    }
                    unsigned long long full = __ballot(cnt > LP_LANE_ITEMS);
                    while (full) {
                        const int j = __ffsll(full) - 1;
                        full &= full - 1;
                        const int cpos = __shfl(pos, j), ccnt = __shfl(cnt, j);
                        const long long ix = lox + (c0 + j) % nx, iy = loy + (c0 + j) / nx;
                        for (int e = lane; e < ccnt; e += 64) n_exp += lp_take(a, X, a.item[cpos + e], ix, iy, w, v2);
                    }
                }
            }
        } else {
            for (int id = lane; id < a.L; id += 64) {
                if (a.elab[id] < 0 || !lp_in_view(a, X, id, v2)) continue;
                n_exp += 1;
                atomicAdd(&a.expected[id], 1);
            }
        }
    }
    n_exp = wave_sum(n_exp);
    n_seen = wave_sum(n_seen);
    if (lane != 0) return;
    a.view[q] = v;
    int32_t* st = a.scan_stat + 4 * (size_t)q;
    st[0] = n_exp;
    st[1] = n_seen;
    st[2] = live;
    st[3] = finite ? 0 : LP_NONFINITE;
    if (has_view) atomicAdd(&a.num[3], 1);
}

__global__ __launch_bounds__(LP_THREADS) void lp_decide_kernel(const LpArgs a) {
    const int i = blockIdx.x * LP_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    bool elig = false, enough = false, retire = false;
    if (i < a.L) {
        const int e = a.expected[i], s = a.seen[i];
        elig = a.elab[i] >= 0;
        enough = elig && e >= a.min_expected;
        retire = enough && (double)s < a.ratio * (double)e;
        a.keep[i] = retire ? 0 : 1;
    }
    const int n0 = __popcll(__ballot(retire)), n1 = __popcll(__ballot(enough)), n2 = __popcll(__ballot(elig));
    if (lane != 0) return;
    if (n0) atomicAdd(&a.num[0], n0);
    if (n1) atomicAdd(&a.num[1], n1);
    if (n2) atomicAdd(&a.num[2], n2);
}

bool lp_size_ok(int Q, int N, int L) { return Q >= 0 && N >= 0 && L >= 0 && (long long)Q * (long long)N <= 0x7fffffffll; }

size_t lp_ws_bytes(size_t L) {
    const size_t h = table_slots(L);
    return align256(L * 4) * 3 + align256(h * 8) + align256(h * 4) * 2 + 256;
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_persist_workspace_bytes(int Q, int N, int L) {
    if (!lp_size_ok(Q, N, L) || Q == 0 || N == 0) return 0;
    return lp_ws_bytes((size_t)L);
}

int sgpr_landmark_persist(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_poses,
                          const int32_t* d_assoc, const double* d_lm_center, const int32_t* d_lm_label,
                          const uint8_t* d_lm_use, int L, const double* h_radius, int n_labels,
                          double max_range, double margin, int min_expected, double max_seen_ratio,
                          int32_t* d_expected, int32_t* d_seen, uint8_t* d_keep, int32_t* d_scan_stat,
                          double* d_view, int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_persist";
    if (!no_negative(fn, {{"Q", Q}, {"N", N}, {"L", L}, {"min_expected", min_expected}})) return SGPR_E_INVALID;
    if (!landmark_labels_ok(fn, h_radius, n_labels) || !radii_ok(fn, h_radius, n_labels)) return SGPR_E_INVALID;
    if (!not_negative(fn, "max_range", max_range)) return SGPR_E_INVALID;
    if (!(margin >= 0.0 && std::isfinite(margin))) {
        set_error(fn + ": margin is negative or not finite");
        return SGPR_E_INVALID;
    }
    if (!(max_seen_ratio >= 0.0 && max_seen_ratio <= 1.0)) {
        set_error(fn + ": max_seen_ratio is NaN or outside [0, 1]");
        return SGPR_E_INVALID;
    }
    if (!lp_size_ok(Q, N, L)) {
        set_error(fn + ": Q N = " + std::to_string((long long)Q * N) + " exceeds the int32 node index");
        return SGPR_E_INVALID;
    }
    if (Q == 0 || N == 0) return SGPR_OK;
    if (!d_centers || !d_labels || !d_poses || !d_assoc || !d_scan_stat || !d_view || !d_num || !d_workspace ||
        ((!d_lm_center || !d_lm_label || !d_expected || !d_seen || !d_keep) && L > 0)) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = lp_ws_bytes((size_t)L);
    if (!workspace_ok(fn, workspace_bytes, need)) return SGPR_E_INVALID;

    Carver ws{static_cast<unsigned char*>(d_workspace)};
    const size_t H = table_slots((size_t)L);
    LpArgs a = {};
    a.centers = d_centers;
    a.labels = d_labels;
    a.poses = d_poses;
    a.assoc = d_assoc;
    a.lm_center = d_lm_center;
    a.lm_label = d_lm_label;
    a.lm_use = d_lm_use;
    a.expected = d_expected;
    a.seen = d_seen;
    a.keep = d_keep;
    a.scan_stat = d_scan_stat;
    a.view = d_view;
    a.num = d_num;
    a.elab = ws.take<int>((size_t)L);
    a.lslot = ws.take<unsigned>((size_t)L);
    a.item = ws.take<int>((size_t)L);
    a.cell_key = ws.take<unsigned long long>(H);
    a.cell_pos = ws.take<int>(H);
    a.cell_cnt = ws.take<int>(H);
    a.total = ws.take<int>(64);
    a.hmask = H - 1;
    a.Q = Q;
    a.N = N;
    a.L = L;
    a.n_labels = n_labels;
    a.min_expected = min_expected;
    a.max_range = max_range;
    a.margin = margin;
    a.ratio = max_seen_ratio;
    a.cell_w = lp_cell_width(max_range, margin);
    for (int l = 0; l < n_labels; ++l) a.radius[l] = h_radius[l];

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(LP_THREADS), lm_grid((L + LP_THREADS - 1) / LP_THREADS);
    if (LP_TABLE && L > 0) {
        // cell_key: empty keys; cell_cnt | total: zero
        hipError_t e = hipMemsetAsync(a.cell_key, 0xff, H * 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(a.cell_cnt, 0, align256(H * 4) + 256, s);
        if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_persist: memset");
    }
    hipLaunchKernelGGL(lp_prep_kernel, dim3(L > 0 ? lm_grid.x : 1), block, 0, s, a);     // (L == 0: d_num alone)
    if (LP_TABLE && L > 0) {
        hipLaunchKernelGGL(lp_offsets_kernel, dim3((unsigned)((H + LP_THREADS - 1) / LP_THREADS)), block, 0, s, a);
        hipLaunchKernelGGL(lp_fill_kernel, lm_grid, block, 0, s, a);
    }
    hipLaunchKernelGGL(lp_tally_kernel<LP_TABLE>, dim3((Q + LP_WAVES - 1) / LP_WAVES), block, 0, s, a);
    if (L > 0) hipLaunchKernelGGL(lp_decide_kernel, lm_grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_persist: launch");
    return SGPR_OK;
}

}  // extern "C"
