// The match-and-fit core of the alignment to a landmark map: what one wave does with one scan and
// one search table - the eligible rule and the cell table of a stage, the match by (d2, id), the scan sums W, the
// closed-form fit and the keep rule of include/sgpr_landmark_align.h.  sgpr_landmark_align.hip runs it once per scan,
// sgpr_landmark_track.hip once per scan and stage, so a stage of the tracker IS an alignment, to the bit.  It is not in
// sgpr_map.hpp: that header holds building blocks many files share (§28), this one the step of one file, declared for
// the two that run it too.  The cell grid and its 9-cell walk, the wave sums, the map point and the closed-form fit it is
// made of are sgpr_map_grid.hpp's.
//
// A scan is read through a small accessor (LaScanGlobal here; the tracker adds one over its LDS copy): both widen the
// same float32 bits, so where the scan lies decides no result.
#pragma once
#include <math.h>

#include "sgpr_internal.hpp"
#include "sgpr_landmarks.h"
#include "sgpr_map_grid.hpp"

namespace sgpr {

#pragma clang fp contract(off)

enum { LA_NONFINITE = 1, LA_KEPT = 2 };

// the landmarks of the map, as the caller passed them
struct LaMap {
    const double* lm_center;
    const int32_t* lm_label;
    const unsigned char* lm_use;
    int L, n_labels;
    double tau_z;
};

// the search structure of one radius table: a slice of the workspace
struct LaTable {
    int* elab;                     // [L] label of an eligible landmark, -1 of any other
    CellGrid g;                    // the eligible landmarks by (label, cell)
};

inline size_t la_table_bytes(size_t L) { return align256(L * 4) + grid_bytes(L); }

// the next la_table_bytes(L) bytes of a workspace
inline LaTable la_table_carve(Carver& ws, size_t L) {
    LaTable t;
    t.elab = ws.take<int>(L);
    t.g = grid_carve(ws, L);
    return t;
}

inline bool la_size_ok(int Q, int N, int L) { return Q >= 0 && N >= 0 && L >= 0 && (long long)Q * (long long)N <= 0x7fffffffll; }

// landmark i under the radii of one table: eligible or not - its label, or -1 - and, with TABLE, an eligible landmark
// enters the cell table and is pushed on its cell's list
template <bool TABLE>
__device__ __forceinline__ void la_prep_landmark(const LaMap& m, const LaTable& t, const double* radius, int i) {
#pragma clang fp contract(off)
    const int l = m.lm_label[i];
    bool ok = (!m.lm_use || m.lm_use[i] != 0) && l >= 0 && l < m.n_labels;
    const double r = ok ? radius[l] : 0.0;
    const double cx = m.lm_center[3 * (size_t)i], cy = m.lm_center[3 * (size_t)i + 1], cz = m.lm_center[3 * (size_t)i + 2];
    ok = ok && r > 0.0 && in_limit37(cx) && in_limit37(cy) && in_limit37(cz);
    t.elab[i] = ok ? l : -1;
    if (!ok || !TABLE) return;
    grid_push(t.g, i, l, lm_cell_width(r), cx, cy);
}

// the match of a map point of label l: landmark o is better than the best so far when it passes the gate and comes
// first by (d2, id)
struct LaBest {
    int id;
    double d2, cx, cy;
};

__device__ __forceinline__ void la_test(const LaMap& m, int o, double mx, double my, double mz, double r2, LaBest& b) {
#pragma clang fp contract(off)
    const double cx = m.lm_center[3 * (size_t)o], cy = m.lm_center[3 * (size_t)o + 1], cz = m.lm_center[3 * (size_t)o + 2];
    const double ex = mx - cx, ey = my - cy;
    const double d2 = ex * ex + ey * ey;
    if (!(d2 <= r2 && fabs(mz - cz) <= m.tau_z)) return;
    if (b.id >= 0 && !(d2 < b.d2 || (d2 == b.d2 && o < b.id))) return;
    b.id = o;
    b.d2 = d2;
    b.cx = cx;
    b.cy = cy;
}

template <bool TABLE>
__device__ __forceinline__ void la_match(const LaMap& m, const LaTable& t, int l, double r, double mx, double my, double mz,
                                         LaBest& b) {
#pragma clang fp contract(off)
    const double r2 = r * r;
    if (TABLE) {
        grid_near(t.g, l, lm_cell_width(r), mx, my, [&](int o) {
            if (t.elab[o] == l) la_test(m, o, mx, my, mz, r2, b);
        });
    } else {
        for (int o = 0; o < m.L; ++o)
            if (t.elab[o] == l) la_test(m, o, mx, my, mz, r2, b);
    }
}

// a scan in global memory: slot n of the packed node arrays
struct LaScanGlobal {
    const float* cen;
    const int32_t* lab;
    __device__ __forceinline__ int label(int n) const { return lab[n]; }
    __device__ __forceinline__ double x(int n) const { return (double)cen[3 * (size_t)n]; }
    __device__ __forceinline__ double y(int n) const { return (double)cen[3 * (size_t)n + 1]; }
    __device__ __forceinline__ double z(int n) const { return (double)cen[3 * (size_t)n + 2]; }
};

// what la_fit_scan leaves behind, the same in every lane but sd2
struct LaFit {
    int matched, live, refits, flags;
    double sd2;                    // this lane's partial of W(d2) under the final pose
};

// sgpr_landmark_align of ONE scan by one whole wave: X is the pose on entry and X_T on return; `row` is the scan's row of
// d_node_landmark, which holds the answer on return.  Lane j owns the slots j, j + 64, ..: exactly partial j of W.  Pass 1
// of a step: the map point of every slot, its match, parked in the row (a lane holds ceil(N / 64) slots: too many for
// registers at any N), and W(p), W(l), W(d2).  Pass 2: the centred moments ar, ai from the parked ids; a lane reads back
// only what it wrote itself.  At k == T, or at the first step that keeps the pose (every later step would keep it too),
// the row already holds the answer.
template <bool TABLE, class Scan>
__device__ __forceinline__ LaFit la_fit_scan(const LaMap& m, const LaTable& t, const double* radius, const Scan& sc, int N, int lane,
                                             int32_t* row, int iters, int min_nodes, Se2& X) {
#pragma clang fp contract(off)
    LaFit f = {0, 0, 0, 0, 0.0};
    if (!se2_finite(X)) {
        for (int n = lane; n < N; n += 64) row[n] = -1;
        f.flags = LA_NONFINITE;
        return f;
    }
    for (int k = 0;; ++k) {
        double spx = 0.0, spy = 0.0, slx = 0.0, sly = 0.0;
        int cnt = 0, lv = 0;
        f.sd2 = 0.0;
        for (int n = lane; n < N; n += 64) {
            const int l = sc.label(n);
            const double x = sc.x(n), y = sc.y(n), mz = sc.z(n);
            double mx, my;
            se2_apply(X, x, y, &mx, &my);
            bool alive = l >= 0 && l < m.n_labels;
            const double r = alive ? radius[l] : 0.0;
            alive = alive && r > 0.0 && in_limit37(mx) && in_limit37(my) && in_limit37(mz);
            LaBest b = {-2, 0.0, 0.0, 0.0};
            if (alive) la_match<TABLE>(m, t, l, r, mx, my, mz, b);
            row[n] = alive ? b.id : -1;
            lv += alive ? 1 : 0;
            if (!alive || b.id < 0) continue;
            cnt += 1;
            spx += x;
            spy += y;
            slx += b.cx;
            sly += b.cy;
            f.sd2 += b.d2;
        }
        f.matched = wave_sum(cnt);
        f.live = wave_sum(lv);
        if (k == iters) break;
        if (f.matched < min_nodes) {
            f.flags |= LA_KEPT;
            break;
        }
        const double dn = (double)f.matched;
        const double pbx = wave_tree(spx) / dn, pby = wave_tree(spy) / dn, lbx = wave_tree(slx) / dn, lby = wave_tree(sly) / dn;
        double ar = 0.0, ai = 0.0;
        for (int n = lane; n < N; n += 64) {
            const int id = row[n];
            if (id < 0) continue;
            const double x = sc.x(n), y = sc.y(n);
            const double lx = m.lm_center[3 * (size_t)id], ly = m.lm_center[3 * (size_t)id + 1];
            const double px = x - pbx, py = y - pby, qx = lx - lbx, qy = ly - lby;
            ar += px * qx + py * qy;
            ai += px * qy - py * qx;
        }
        ar = wave_tree(ar);
        ai = wave_tree(ai);
        const Se2Fit fit = se2_fit(pbx, pby, lbx, lby, ar, ai);
        if (fit.degenerate()) {                                 // (the same bits in every lane: a uniform branch)
            f.flags |= LA_KEPT;
            break;
        }
        X = fit.F;
        ++f.refits;
    }
    return f;
}

// d_rms of a fitted scan: sqrt(W(d2) / matched), the quiet NaN without a match; every lane of the wave calls it
__device__ __forceinline__ double la_rms(const LaFit& f) {
#pragma clang fp contract(off)
    const double total = wave_tree(f.sd2);
    return f.matched > 0 ? sqrt(total / (double)f.matched) : __longlong_as_double(0x7ff8000000000000ll);
}

}  // namespace sgpr
