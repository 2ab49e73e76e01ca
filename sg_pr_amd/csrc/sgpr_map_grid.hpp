// The building blocks the LANDMARK back end shares, on top of sgpr_map.hpp: the fixed-point constants and
// the 2^37 limit, the wave sums, the map point, the per-label cell grid (push, and the walk of the 9 cells around a
// point), the linking step of the two fusing sequences, the numbering of roots and the closed-form planar fit.  One
// definition of each; the eight sgpr_landmark*.hip files include it.
//
// Floating-point contraction: as in sgpr_map.hpp, every function here that multiplies and adds carries the pragma in
// its own body.
#pragma once
#include <type_traits>

#include "sgpr_landmarks.h"
#include "sgpr_map.hpp"

namespace sgpr {

// ------------------------------------------------------------------ constants of the record arithmetic
constexpr double MAP_FIX = 16777216.0;             // 2^24: one unit of the fixed-point sums
constexpr double MAP_LIMIT = 137438953472.0;       // 2^37: |coordinate| of a live map point / an eligible centre
constexpr double MAP_D2_CAP = 1048576.0;           // 2^20: cap of a squared distance (a variance) before it is summed
constexpr int MAP_MAX_COUNT = 262144;              // 2^18: count of an eligible record
constexpr double MAP_SUM_LIMIT = 274877906944.0;   // 2^38: |centre count| of an eligible record

__device__ __forceinline__ bool in_limit37(double v) { return isfinite(v) && fabs(v) <= MAP_LIMIT; }

// ELIGIBLE of include/sgpr_landmark_update.h and include/sgpr_landmark_merge.h, on one record (c: its centre, moved or
// not); `radius` is the table in the kernel's arguments
__device__ __forceinline__ bool record_eligible(int l, int n, double sp, double cx, double cy, double cz, const double* radius,
                                                int n_labels) {
#pragma clang fp contract(off)
    const double n0 = (double)n;
    bool ok = l >= 0 && l < n_labels && n >= 1 && n <= MAP_MAX_COUNT;
    ok = ok && radius[ok ? l : 0] > 0.0;
    ok = ok && isfinite(sp) && sp >= 0.0;
    return ok && isfinite(cx) && fabs(cx * n0) <= MAP_SUM_LIMIT && isfinite(cy) && fabs(cy * n0) <= MAP_SUM_LIMIT && isfinite(cz) &&
           fabs(cz * n0) <= MAP_SUM_LIMIT;
}

// ------------------------------------------------------------------ sums over a wave
// the halving tree of W over the 64 partials of a wave; every lane gets v[0].  The ORDER of these additions defines the
// bits of W (include/sgpr_landmark_refine.h, include/sgpr_landmark_align.h): it is not to be rearranged.
__device__ __forceinline__ double wave_tree(double v) {
    for (int h = 32; h > 0; h >>= 1) v += __shfl_down(v, h);    // (lanes i < h hold v[i] + v[i + h]; the others are not read)
    return __shfl(v, 0);
}
// the sum of an integer over the wave, in every lane (any order, same sum)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int h = 32; h > 0; h >>= 1) v += __shfl_down(v, h);
    return __shfl(v, 0);
}

// ------------------------------------------------------------------ the map point
// (x, y) of a sensor frame under X: (c x - s y) + X, (s x + c y) + Y, every operation rounded on its own.  Both are formed
// before either is stored: mx, my may be the caller's x, y.
__device__ __forceinline__ void se2_apply(const Se2& X, double x, double y, double* mx, double* my) {
#pragma clang fp contract(off)
    const double u = (X.c * x - X.s * y) + X.x, v = (X.s * x + X.c * y) + X.y;
    *mx = u;
    *my = v;
}

// ------------------------------------------------------------------ the closed-form planar fit
// From the four means (p: sensor frame, l: map frame) and the two centred moments, all reduced by wave_tree: the
// rotation (ar, ai) / h and the translation that maps the one mean onto the other.  Whether the pose is then kept
// (fixed scans, too few nodes, where the iteration stops) is the caller's rule.
struct Se2Fit {
    Se2 F;
    double h;
    // no rotation can be told (h is 0 or not finite) or the fit is not finite; the same bits in every lane
    __device__ __forceinline__ bool degenerate() const { return !(h > 0.0 && isfinite(h)) || !se2_finite(F); }
};

__device__ __forceinline__ Se2Fit se2_fit(double pbx, double pby, double lbx, double lby, double ar, double ai) {
#pragma clang fp contract(off)
    Se2Fit f;
    f.h = sqrt(ar * ar + ai * ai);
    f.F.c = ar / f.h;
    f.F.s = ai / f.h;
    f.F.x = lbx - (f.F.c * pbx - f.F.s * pby);
    f.F.y = lby - (f.F.s * pbx + f.F.c * pby);
    return f;
}

// ------------------------------------------------------------------ the cell grid: a list per (label, cell)
// The items 0 .. n - 1 of a grid are points of the map frame; an item is pushed on the list of its cell - the cell of
// its label's width (lm_cell_width; any width the caller's proof allows) - and the lists are walked by a later kernel.
struct CellGrid {
    int* next;                     // [n] linked list of the item's cell
    unsigned long long* cell_key;  // [H] (sgpr_map.hpp's open-addressing table)
    int* cell_head;                // [H] first item of the cell's list, -1: none
    unsigned long long hmask;      // H - 1 (H = table_slots(n))
};

// cell_key | cell_head are contiguous: ONE memset of 0xff over grid_clear_bytes(n) from cell_key gives empty keys and
// list ends
inline size_t grid_clear_bytes(size_t n) { return align256(table_slots(n) * 8) + align256(table_slots(n) * 4); }
inline size_t grid_bytes(size_t n) { return align256(n * 4) + grid_clear_bytes(n); }
// the next grid_bytes(n) bytes of a workspace
inline CellGrid grid_carve(Carver& ws, size_t n) {
    const size_t H = table_slots(n);
    CellGrid g;
    g.next = ws.take<int>(n);
    g.cell_key = ws.take<unsigned long long>(H);
    g.cell_head = ws.take<int>(H);
    g.hmask = H - 1;
    return g;
}

// the table slot of the cell of (x, y) under `label`, entered when absent
__device__ __forceinline__ unsigned long long grid_cell_slot(unsigned long long* cell_key, unsigned long long hmask, int label,
                                                             double cell_width, double x, double y) {
    return table_insert(cell_key, hmask, lm_cell_key(label, lm_cell_coord(x, cell_width), lm_cell_coord(y, cell_width)));
}

// item i at (x, y) enters the table and is pushed on its cell's list.  The order of a list is whatever the atomics make it.
__device__ __forceinline__ void grid_push(const CellGrid& g, int i, int label, double cell_width, double x, double y) {
    const unsigned long long slot = grid_cell_slot(g.cell_key, g.hmask, label, cell_width, x, y);
    g.next[i] = atomicExch(&g.cell_head[slot], i);
}

// f(o) for every item o on the lists of the 9 cells around (x, y); f returns whether to stop, or nothing when it never
// does (the walk then has no way out but its end, which keeps the loops over the cells uniform).  -> stopped.
// With the label's own width every item in range of (x, y) is among them (lm_cell_width's proof).  A SHARED LIST:
// lm_cell_key is a hash, so two cells may share one list and a list may be met twice among the 9; f compares the labels
// and the distance itself, and what follows from a hit (uniting, a minimum, "one exists") is idempotent, so a collision
// costs time and never an answer.
template <class F>
__device__ __forceinline__ bool grid_near(const CellGrid& g, int label, double cell_width, double x, double y, F&& f) {
    const long long ix = lm_cell_coord(x, cell_width), iy = lm_cell_coord(y, cell_width);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const unsigned long long slot = table_find(g.cell_key, g.hmask, lm_cell_key(label, ix + dx, iy + dy));
            if (slot == TABLE_EMPTY) continue;
            for (int o = g.cell_head[slot]; o >= 0; o = g.next[o]) {
                if constexpr (std::is_void<decltype(f(o))>::value) f(o);
                else if (f(o)) return true;
            }
        }
    return false;
}

// ------------------------------------------------------------------ the linking step of a fusing sequence
// Item i of label lab[i] at pts[3 i ..]: the lower-indexed items of its label on the lists of its 9 cells are tested
// with the rule of include/sgpr_landmarks.h - planar distance within the label's radius, heights within tau_z - and
// united, every unordered pair once.  The larger root is hooked under the smaller (uf_unite), so a component's root is
// its lowest index whatever the execution order.  lab[i] < 0: the item takes no part.
__device__ __forceinline__ void link_item(const CellGrid& g, const double* pts, const int* lab, int* parent, const double* radius,
                                          double tau_z, int i) {
#pragma clang fp contract(off)
    const int l = lab[i];
    if (l < 0) return;
    const double r = radius[l], r2 = r * r;
    const double cw = lm_cell_width(r);
    const double mx = pts[3 * (size_t)i], my = pts[3 * (size_t)i + 1], mz = pts[3 * (size_t)i + 2];
    grid_near(g, l, cw, mx, my, [&](int o) {
        if (o >= i || lab[o] != l) return;
        const double ex = mx - pts[3 * (size_t)o], ey = my - pts[3 * (size_t)o + 1];
        const double d2 = ex * ex + ey * ey;
        if (d2 <= r2 && fabs(mz - pts[3 * (size_t)o + 2]) <= tau_z) uf_unite(parent, i, o);
    });
}

// ------------------------------------------------------------------ the numbering of roots
// id of a root = the roots before it = (roots of the workgroups before its own) + (its rank inside its workgroup).
// A numbered kernel has NUMBER_THREADS threads a workgroup; the counts of the B workgroups are scanned by one workgroup
// of SCAN_THREADS.
constexpr int NUMBER_THREADS = 256;
constexpr int SCAN_THREADS = 1024;

// the number of flagged threads of the workgroup, valid in thread 0; wsum: NUMBER_THREADS / 64 ints of LDS
__device__ __forceinline__ int block_count(bool flag, int* wsum) {
    const unsigned long long ball = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(ball);
    __syncthreads();
    int s = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < NUMBER_THREADS / 64; ++i) s += wsum[i];
    return s;
}

// One workgroup of SCAN_THREADS: blk[0 .. B) becomes its exclusive prefix sum.  Thread t owns the segment of
// ceil(B / SCAN_THREADS) counts from t times that (longer than one entry once B > SCAN_THREADS); the segment sums are
// scanned in LDS.  TWO: blk2 is summed along (it is not rewritten).  Afterwards part[SCAN_THREADS - 1] (and
// part2[SCAN_THREADS - 1]) holds the total, readable by that thread: where it goes is the caller's business.
template <bool TWO>
__device__ __forceinline__ void scan_block_counts(int* blk, const int* blk2, int B, int* part, int* part2) {
    const int t = threadIdx.x;
    const int seg = (B + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min(t * seg, B), hi = min(lo + seg, B);
    int s = 0, s2 = 0;
    for (int i = lo; i < hi; ++i) {
        s += blk[i];
        if (TWO) s2 += blk2[i];
    }
    part[t] = s;
    if (TWO) part2[t] = s2;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {          // inclusive scan of the segment sums
        const int u = t >= off ? part[t - off] : 0, v = TWO && t >= off ? part2[t - off] : 0;
        __syncthreads();
        part[t] += u;
        if (TWO) part2[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = lo; i < hi; ++i) {
        const int c = blk[i];
        blk[i] = run;
        run += c;
    }
}

// the rank of a flagged thread among the flagged threads of its workgroup (of an unflagged one: no meaning).  Every
// thread of the workgroup calls it: it holds a barrier.  wcount: NUMBER_THREADS / 64 ints of LDS
__device__ __forceinline__ int rank_in_block(bool flag, int* wcount) {
    const unsigned long long ball = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wcount[wave] = __popcll(ball);
    __syncthreads();
    int rank = __popcll(ball & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) rank += wcount[v];
    return rank;
}

// ------------------------------------------------------------------ host: the radius tables of the landmark entry points
// (with sgpr_map.hpp's argument checks: false, and the message is set)
// n_labels in range and a radius table given; `name` is the table's in the message
inline bool landmark_labels_ok(const std::string& fn, const double* h_radius, int n_labels, const char* name = "h_radius") {
    if (n_labels < 1 || n_labels > SGPR_LANDMARK_MAX_LABELS) {
        set_error(fn + ": n_labels " + std::to_string(n_labels) + " outside [1, " + std::to_string(SGPR_LANDMARK_MAX_LABELS) + "]");
        return false;
    }
    if (!h_radius) {
        set_error(fn + ": NULL " + name);
        return false;
    }
    return true;
}
// every radius of one table is >= 0; `what` words it ("radius", "inlier radius"), stage >= 0 adds the stage of a schedule
inline bool radii_ok(const std::string& fn, const double* h_radius, int n_labels, const char* what = "radius", int stage = -1) {
    for (int l = 0; l < n_labels; ++l)
        if (!(h_radius[l] >= 0.0)) {
            set_error(fn + ": " + what + " of label " + std::to_string(l) + (stage >= 0 ? " in stage " + std::to_string(stage) : std::string()) +
                      " is negative or NaN");
            return false;
        }
    return true;
}

}  // namespace sgpr
