// Relocalise scans in a landmark map with no prior pose (sgpr_landmark_relocalize; include/sgpr_landmark_relocalize.h,
// DESIGN.md §35): pairs of scan nodes hypothesised onto pairs of landmarks of their labels, the hypothesis with the
// largest consensus, the best consensus at another place, and the winner refined by a schedule of alignment gates.
// Float64 with every operation rounded on its own.  A refine stage is sgpr_landmark_align of one scan, and it is the
// same code: la_fit_scan of sgpr_landmark_align_core.hpp, which la_align_kernel and lt_track_kernel run too.
//
//   lr_prep_kernel    one thread per landmark, one launch per table (the radii of a table ride in the launch).  Launch 0:
//                     eligible or not under h_radius_in, the cell table of the inlier test, the PAIR table - cells
//                     lm_cell_width(max_base + tau_edge) wide, so the nine cells around landmark j hold every j' a
//                     hypothesis can pair it with (§28's proof with that radius) - and the number of eligible landmarks
//                     per label.  Launch 1 + k: the table of refine stage k, and its radii into the workspace.
//   lr_list_kernel    the eligible landmarks grouped by label: a landmark takes the next free place of its label's range.
//                     The order inside a range is whatever the atomics give; nothing below depends on it.
//   lr_reloc_kernel   one workgroup of 256 threads per scan.  The scan is staged in LDS when N <= LR_LDS_SLOTS and read
//                     through align's global accessor otherwise; its live slots are compacted in slot order.
//       enumerate     a workgroup-uniform loop over the base pairs in ascending (i, i'); the running hypothesis count is
//                     the same register value in every lane, so the cap is one uniform comparison.  Per base pair the
//                     landmarks j of label(i) are taken 256 at a time, one per lane; a lane walks the nine pair-table
//                     cells around its j as a cursor and stops at its next admissible j'.  A ROUND appends what the lanes
//                     found - at most one entry each - to a batch in LDS: positions from a ballot per wave and four
//                     per-wave counts (two sets, alternating: one barrier per round).  A landmark is taken only from the
//                     walked cell that is ITS cell, so two cells that share a list (lm_cell_key is a hash) or a list met
//                     twice never count a hypothesis twice.
//       evaluate      when the batch holds LR_FLUSH entries, and at the end of every base pair, the waves take its
//                     entries in turn: ONE HYPOTHESIS PER WAVE, lanes over the live nodes.  The pose is wave-uniform, the
//                     count is a popcount of a ballot, and a base pair's handful of hypotheses keeps all four waves busy
//                     (one hypothesis per lane would need 256 of them before it paid).  A wave keeps its best key.
//       other place   a second enumeration when the scan is FOUND: the set evaluated is fixed by the cap rule, so it is
//                     the same set; hypotheses within `sep` of the winner are skipped before they are counted.
//       refine        wave 0 runs the stages through la_fit_scan; lane 0 writes the scan's outputs.
//
// Every loop is bounded by slot counts, list lengths and the cap (a base pair adds at most L^2 past it).  No wave waits
// for another workgroup.  Integer atomics only, no inline assembly, plain vector stores.
//
// Both tables are sgpr_map_grid.hpp's cell grid: landmarks enter them by grid_push, and the inlier test (lr_exists) is
// grid_near with a way out at the first hit.  The cursor over the pair table stays written out: a lane must be able to
// stop in the middle of a list and go on in the next round, which a visitor cannot.
#include <math.h>

#include <cmath>
#include <string>
#include <type_traits>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_align_core.hpp"
#include "sgpr_landmark_relocalize.h"
#include "sgpr_map_grid.hpp"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_WAVES = LR_THREADS / 64;
constexpr int LR_LDS_SLOTS = 256;              // slots of a scan the workgroup stages: 256 x 16 bytes = 4 KiB
constexpr int LR_FLUSH = 256;                  // entries of the batch that start an evaluation
constexpr int LR_BATCH = 2 * LR_FLUSH;         // fewer than LR_FLUSH left over + at most LR_THREADS appended by a round
constexpr int LR_LABELS = SGPR_LANDMARK_MAX_LABELS;

struct LrPrepArgs {
    LaMap m;
    LaTable t;                                 // the table of this launch
    LaTable pair;                              // launch 0: the pair table (its elab is not written here)
    int* lab_count;                            // launch 0: [LR_LABELS] eligible landmarks per label
    double* radius_out;                        // launches 1 + k: [LR_LABELS] the stage's radii in the workspace
    double pair_r;                             // max_base + tau_edge
    int with_pair;
    double radius[LR_LABELS];
};

struct LrArgs {
    const float* centers;
    const int32_t* labels;
    LaMap m;
    LaTable t_in;                              // under h_radius_in
    LaTable pair;                              // next | cell_key | cell_head of the pair table
    LaTable t[SGPR_RELOC_MAX_STAGES];
    const int* list;                           // [L] eligible landmarks grouped by label
    const int* lab_count;                      // [LR_LABELS]
    const double* stage_radius;                // [n_stages][LR_LABELS]
    int* live;                                 // [Q N] when N > LR_LDS_SLOTS
    double* poses_out;
    double* coarse;
    double* other;
    int32_t* node_landmark;
    int32_t* stat;
    int32_t* win;
    long long* hyp;
    double* rms;
    int32_t* num;
    int Q, N, n_stages, max_hyp, min_inliers, iters, min_nodes;
    double tau_edge, min_base, max_base, sep2, pair_r;
    double radius_in[LR_LABELS];
};

__global__ __launch_bounds__(LR_THREADS) void lr_prep_kernel(const LrPrepArgs a) {
    const int i = blockIdx.x * LR_THREADS + threadIdx.x;
    if (a.radius_out && i < a.m.n_labels) a.radius_out[i] = a.radius[i];
    if (i >= a.m.L) return;
    la_prep_landmark<true>(a.m, a.t, a.radius, i);
    const int l = a.t.elab[i];
    if (!a.with_pair || l < 0) return;
    grid_push(a.pair.g, i, l, lm_cell_width(a.pair_r), a.m.lm_center[3 * (size_t)i], a.m.lm_center[3 * (size_t)i + 1]);
    atomicAdd(&a.lab_count[l], 1);
}

// lab_count | lab_cursor are contiguous; list is the pair table's elab slice
__global__ __launch_bounds__(LR_THREADS) void lr_list_kernel(const int* elab, int L, int* lab_count, int* list) {
    const int i = blockIdx.x * LR_THREADS + threadIdx.x;
    if (i >= L) return;
    const int l = elab[i];
    if (l < 0) return;
    int start = 0;
    for (int k = 0; k < l; ++k) start += lab_count[k];
    list[start + atomicAdd(&lab_count[LR_LABELS + l], 1)] = i;
}

// a scan in the workgroup's LDS: (x, y, z, label) bits per slot
struct LrScanLds {
    const int4* p;
    __device__ __forceinline__ int label(int n) const { return p[n].w; }
    __device__ __forceinline__ double x(int n) const { return (double)__int_as_float(p[n].x); }
    __device__ __forceinline__ double y(int n) const { return (double)__int_as_float(p[n].y); }
    __device__ __forceinline__ double z(int n) const { return (double)__int_as_float(p[n].z); }
};

// the key of a hypothesis: inliers descending, then i, i', j, j' ascending; inl < 0: none
struct LrKey {
    int inl, i, ip, j, jp;
};

__device__ __forceinline__ bool lr_better(const LrKey& a, const LrKey& b) {
    if (a.inl != b.inl) return a.inl > b.inl;
    if (a.i != b.i) return a.i < b.i;
    if (a.ip != b.ip) return a.ip < b.ip;
    if (a.j != b.j) return a.j < b.j;
    return a.jp < b.jp;
}

// what a base pair gives every one of its hypotheses
struct LrBase {
    double xi, yi, zi, xp, yp, zp, ux, uy, lu;
};

// the coarse pose of (base, j, j') from the two centres; false: no hypothesis
__device__ __forceinline__ bool lr_pose(const LrBase& b, double cx, double cy, double dx, double dy, double tau_edge, Se2& X) {
#pragma clang fp contract(off)
    const double vx = dx - cx, vy = dy - cy;
    const double lv = sqrt(vx * vx + vy * vy);
    if (!(fabs(b.lu - lv) <= tau_edge)) return false;
    const double den = b.lu * lv;
    if (!(den > 0.0 && isfinite(den))) return false;
    X.c = (b.ux * vx + b.uy * vy) / den;
    X.s = (b.ux * vy - b.uy * vx) / den;
    const double pmx = 0.5 * (b.xi + b.xp), pmy = 0.5 * (b.yi + b.yp);
    const double lmx = 0.5 * (cx + dx), lmy = 0.5 * (cy + dy);
    X.x = lmx - (X.c * pmx - X.s * pmy);
    X.y = lmy - (X.s * pmx + X.c * pmy);
    return se2_finite(X);
}

// does a MATCH exist for a map point of label l: la_match's walk, left at the first landmark inside the gate
__device__ __forceinline__ bool lr_exists(const LaMap& m, const LaTable& t, int l, double r, double mx, double my, double mz) {
#pragma clang fp contract(off)
    const double r2 = r * r;
    return grid_near(t.g, l, lm_cell_width(r), mx, my, [&](int o) {
        if (t.elab[o] != l) return false;
        const double cx = m.lm_center[3 * (size_t)o], cy = m.lm_center[3 * (size_t)o + 1], cz = m.lm_center[3 * (size_t)o + 2];
        const double ex = mx - cx, ey = my - cy;
        return ex * ex + ey * ey <= r2 && fabs(mz - cz) <= m.tau_z;
    });
}

template <bool LDS>
__global__ __launch_bounds__(LR_THREADS) void lr_reloc_kernel(const LrArgs a) {
    __shared__ int4 staged[LDS ? LR_LDS_SLOTS : 1];
    __shared__ int live_lds[LDS ? LR_LDS_SLOTS : 1];
    __shared__ int2 batch[LR_BATCH];
    __shared__ int wcnt[2][LR_WAVES];
    __shared__ LrKey wkey[LR_WAVES];
    __shared__ int lstart[LR_LABELS + 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x, N = a.N;
    const size_t base = (size_t)q * (size_t)N;
    const float* cen = a.centers + 3 * base;
    const int32_t* lab = a.labels + base;
    const unsigned long long below = (1ull << lane) - 1ull;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    if (LDS)
        for (int n = tid; n < N; n += LR_THREADS)
            staged[n] = make_int4(__float_as_int(cen[3 * (size_t)n]), __float_as_int(cen[3 * (size_t)n + 1]),
                                  __float_as_int(cen[3 * (size_t)n + 2]), lab[n]);
    if (tid == 0) {
        int s = 0;
        for (int l = 0; l < LR_LABELS; ++l) {
            lstart[l] = s;
            s += l < a.m.n_labels ? a.lab_count[l] : 0;
        }
        lstart[LR_LABELS] = s;
    }
    __syncthreads();
    using Scan = typename std::conditional<LDS, LrScanLds, LaScanGlobal>::type;
    Scan sc;
    if constexpr (LDS) sc = LrScanLds{staged};
    else sc = LaScanGlobal{cen, lab};
    int* live = LDS ? live_lds : a.live + base;

    auto node_live = [&](int n) {
        const int l = sc.label(n);
        if (!(l >= 0 && l < a.m.n_labels)) return false;
        return a.radius_in[l] > 0.0 && in_limit37(sc.x(n)) && in_limit37(sc.y(n)) && in_limit37(sc.z(n));
    };

    // ---- the live slots, in slot order
    int par = 0, nl = 0;
    for (int n0 = 0; n0 < N; n0 += LR_THREADS) {
        const int n = n0 + tid;
        const bool alive = n < N && node_live(n);
        const unsigned long long bal = __ballot(alive);
        if (lane == 0) wcnt[par][wave] = __popcll(bal);
        int pos = nl + __popcll(bal & below);
        __syncthreads();
        int added = 0;
#pragma unroll
        for (int w = 0; w < LR_WAVES; ++w) {
            const int c = wcnt[par][w];
            if (w < wave) pos += c;
            added += c;
        }
        if (alive) live[pos] = n;
        nl += added;
        par ^= 1;
    }
    __syncthreads();

    const double cw = lm_cell_width(a.pair_r);

    // one pass over the base pairs and their hypotheses.  second: only hypotheses farther than sep from (wx, wy) are
    // evaluated.  Every value it returns is the same in every lane but `best`, which is the wave's.
    unsigned long long tail = 0;
    int started = 0;
    bool truncated = false;
    auto enumerate = [&](bool second, double wx, double wy, LrKey& best) {
        tail = 0;
        started = 0;
        truncated = false;
        best = LrKey{-1, 0, 0, 0, 0};
        int cnt = 0;                                            // entries of the batch (uniform)
        LrBase b;
        int si = 0, sp = 0;

        auto evaluate = [&]() {
            for (int e = wave; e < cnt; e += LR_WAVES) {
                const int2 h = batch[e];
                const double cx = a.m.lm_center[3 * (size_t)h.x], cy = a.m.lm_center[3 * (size_t)h.x + 1];
                const double dx = a.m.lm_center[3 * (size_t)h.y], dy = a.m.lm_center[3 * (size_t)h.y + 1];
                Se2 X;
                lr_pose(b, cx, cy, dx, dy, a.tau_edge, X);      // (admissible: the enumeration formed the same bits)
                if (second) {
                    const double ex = X.x - wx, ey = X.y - wy;
                    if (!(ex * ex + ey * ey > a.sep2)) continue;
                }
                int inl = 0;
                for (int n0 = 0; n0 < nl; n0 += 64) {
                    bool hit = false;
                    if (n0 + lane < nl) {
                        const int n = live[n0 + lane];
                        const int l = sc.label(n);
                        const double x = sc.x(n), y = sc.y(n), mz = sc.z(n);
                        double mx, my;
                        se2_apply(X, x, y, &mx, &my);
                        hit = in_limit37(mx) && in_limit37(my) && lr_exists(a.m, a.t_in, l, a.radius_in[l], mx, my, mz);
                    }
                    inl += __popcll(__ballot(hit));
                }
                const LrKey k = {inl, si, sp, h.x, h.y};
                if (lr_better(k, best)) best = k;
            }
        };

        for (int i0 = 0; i0 < nl && !truncated; ++i0) {
            si = live[i0];
            const int li = sc.label(si);
            b.xi = sc.x(si);
            b.yi = sc.y(si);
            b.zi = sc.z(si);
            const int j_lo = lstart[li], nj = lstart[li + 1] - j_lo;
            for (int i1 = i0 + 1; i1 < nl; ++i1) {
                sp = live[i1];
                b.xp = sc.x(sp);
                b.yp = sc.y(sp);
                b.zp = sc.z(sp);
                b.ux = b.xp - b.xi;
                b.uy = b.yp - b.yi;
                b.lu = sqrt(b.ux * b.ux + b.uy * b.uy);
                if (!(a.min_base <= b.lu && b.lu <= a.max_base)) continue;
                if (tail >= (unsigned long long)a.max_hyp) {
                    truncated = true;
                    break;
                }
                started += started < 0x7fffffff ? 1 : 0;     // (d_stat[q][6] saturates)
                const int lp = sc.label(sp);
                if (lstart[lp + 1] == lstart[lp]) continue;     // (no landmark of label(i'): the pair contributes nothing)
                for (int c0 = 0; c0 < nj; c0 += LR_THREADS) {
                    // this lane's j, and its cursor over the nine cells around it
                    bool active = c0 + tid < nj;
                    int j = -1, k = 0, o = -1;
                    double cx = 0.0, cy = 0.0;
                    long long ix = 0, iy = 0, wx_ = 0, wy_ = 0;
                    if (active) {
                        j = a.list[j_lo + c0 + tid];
                        cx = a.m.lm_center[3 * (size_t)j];
                        cy = a.m.lm_center[3 * (size_t)j + 1];
                        active = fabs(b.zi - a.m.lm_center[3 * (size_t)j + 2]) <= a.m.tau_z;
                        ix = lm_cell_coord(cx, cw);
                        iy = lm_cell_coord(cy, cw);
                    }
                    while (true) {
                        bool found = false;
                        int jp = -1;
                        while (active) {
                            if (o < 0) {
                                if (k == 9) {
                                    active = false;
                                    break;
                                }
                                wx_ = ix + (k % 3 - 1);
                                wy_ = iy + (k / 3 - 1);
                                ++k;
                                const unsigned long long slot = table_find(a.pair.g.cell_key, a.pair.g.hmask, lm_cell_key(lp, wx_, wy_));
                                o = slot == TABLE_EMPTY ? -1 : a.pair.g.cell_head[slot];
                                continue;
                            }
                            const int cand = o;
                            o = a.pair.g.next[cand];
                            if (cand == j || a.t_in.elab[cand] != lp) continue;
                            const double dx = a.m.lm_center[3 * (size_t)cand], dy = a.m.lm_center[3 * (size_t)cand + 1];
                            if (lm_cell_coord(dx, cw) != wx_ || lm_cell_coord(dy, cw) != wy_) continue;   // (not ITS cell)
                            if (!(fabs(b.zp - a.m.lm_center[3 * (size_t)cand + 2]) <= a.m.tau_z)) continue;
                            Se2 X;
                            if (!lr_pose(b, cx, cy, dx, dy, a.tau_edge, X)) continue;
                            found = true;
                            jp = cand;
                            break;
                        }
                        const unsigned long long bal = __ballot(found);
                        if (lane == 0) wcnt[par][wave] = __popcll(bal);
                        int pos = cnt + __popcll(bal & below);
                        // (the position needs the other waves' counts: the entry is written after the barrier, into a
                        //  place no lane reads before the next barrier)
                        __syncthreads();
                        int added = 0;
#pragma unroll
                        for (int w = 0; w < LR_WAVES; ++w) {
                            const int c = wcnt[par][w];
                            if (w < wave) pos += c;
                            added += c;
                        }
                        if (found) batch[pos] = make_int2(j, jp);
                        cnt += added;
                        tail += (unsigned long long)added;
                        par ^= 1;
                        if (added == 0) break;                  // (no lane found one: every cursor is at its end)
                        if (cnt >= LR_FLUSH) {
                            __syncthreads();                    // the entries of this round are in the batch
                            evaluate();
                            cnt = 0;
                        }
                    }
                }
                if (cnt > 0) {                                  // a base pair's last entries: the next one has other nodes
                    __syncthreads();
                    evaluate();
                    cnt = 0;
                }
            }
        }
    };

    // the workgroup's best of the waves' bests: the same in every lane
    auto reduce = [&](const LrKey& mine) {
        __syncthreads();                                        // (wkey of an earlier reduction has been read)
        if (lane == 0) wkey[wave] = mine;
        __syncthreads();
        LrKey k = wkey[0];
#pragma unroll
        for (int w = 1; w < LR_WAVES; ++w)
            if (lr_better(wkey[w], k)) k = wkey[w];
        return k;
    };

    auto pose_of = [&](const LrKey& k) {
        LrBase b;
        b.xi = sc.x(k.i);
        b.yi = sc.y(k.i);
        b.zi = sc.z(k.i);
        b.xp = sc.x(k.ip);
        b.yp = sc.y(k.ip);
        b.zp = sc.z(k.ip);
        b.ux = b.xp - b.xi;
        b.uy = b.yp - b.yi;
        b.lu = sqrt(b.ux * b.ux + b.uy * b.uy);
        Se2 X;
        lr_pose(b, a.m.lm_center[3 * (size_t)k.j], a.m.lm_center[3 * (size_t)k.j + 1], a.m.lm_center[3 * (size_t)k.jp],
                a.m.lm_center[3 * (size_t)k.jp + 1], a.tau_edge, X);
        return X;
    };

    LrKey mine;
    enumerate(false, 0.0, 0.0, mine);
    const LrKey win = reduce(mine);
    const unsigned long long hyps = tail;
    const int base_pairs = started;
    const bool was_cut = truncated;
    const bool any = win.inl >= 0;
    const bool found = any && win.inl >= a.min_inliers;
    Se2 C = {qnan, qnan, qnan, qnan};
    if (any) C = pose_of(win);
    LrKey oth = {-1, 0, 0, 0, 0};
    if (found) {                                                // (uniform)
        enumerate(true, C.x, C.y, mine);
        oth = reduce(mine);
    }
    if (wave != 0) return;

    // ---- refinement and outputs: wave 0
    int32_t* row = a.node_landmark + base;
    Se2 X = C;
    LaFit f = {0, nl, 0, 0, 0.0};
    int refits = 0, flags = (found ? SGPR_RELOC_FOUND : 0) | (was_cut ? SGPR_RELOC_TRUNCATED : 0) | (any ? 0 : SGPR_RELOC_NO_HYPOTHESIS);
    double rms = qnan;
    if (found) {
        if (a.n_stages == 0) f = la_fit_scan<true>(a.m, a.t_in, a.radius_in, sc, N, lane, row, 0, a.min_nodes, X);
        for (int s = 0; s < a.n_stages; ++s) {
            f = la_fit_scan<true>(a.m, a.t[s], a.stage_radius + (size_t)s * LR_LABELS, sc, N, lane, row, a.iters, a.min_nodes, X);
            refits += f.refits;
            flags |= (f.flags & LA_KEPT) ? SGPR_RELOC_KEPT : 0;
        }
        rms = la_rms(f);
    } else {
        for (int n = lane; n < N; n += 64) row[n] = node_live(n) ? -2 : -1;
        X = Se2{qnan, qnan, qnan, qnan};
    }
    if (lane != 0) return;
    Se2 O = {qnan, qnan, qnan, qnan};
    if (oth.inl >= 0) O = pose_of(oth);
    double* po = a.poses_out + 4 * (size_t)q;
    double* pc = a.coarse + 4 * (size_t)q;
    double* pt = a.other + 4 * (size_t)q;
    po[0] = X.c, po[1] = X.s, po[2] = X.x, po[3] = X.y;
    pc[0] = C.c, pc[1] = C.s, pc[2] = C.x, pc[3] = C.y;
    pt[0] = O.c, pt[1] = O.s, pt[2] = O.x, pt[3] = O.y;
    int32_t* st = a.stat + 8 * (size_t)q;
    st[0] = any ? win.inl : 0;
    st[1] = oth.inl >= 0 ? oth.inl : 0;
    st[2] = f.matched;
    st[3] = f.live;
    st[4] = refits;
    st[5] = flags;
    st[6] = base_pairs;
    st[7] = 0;
    int32_t* w = a.win + 4 * (size_t)q;
    w[0] = any ? win.i : -1;
    w[1] = any ? win.ip : -1;
    w[2] = any ? win.j : -1;
    w[3] = any ? win.jp : -1;
    a.hyp[q] = (long long)hyps;
    a.rms[q] = rms;
    if (found) atomicAdd(&a.num[0], 1);
    if (was_cut) atomicAdd(&a.num[1], 1);
    if (!any) atomicAdd(&a.num[2], 1);
}

bool lr_stages_ok(int n_stages) { return n_stages >= 0 && n_stages <= SGPR_RELOC_MAX_STAGES; }

size_t lr_workspace(int Q, int N, int L, int n_stages) {
    return (size_t)(n_stages + 2) * la_table_bytes((size_t)L) + align256(2 * LR_LABELS * sizeof(int)) +
           align256((size_t)n_stages * LR_LABELS * sizeof(double)) +
           (N > LR_LDS_SLOTS ? align256((size_t)Q * (size_t)N * sizeof(int)) : 0);
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_relocalize_workspace_bytes(int Q, int N, int L, int n_stages) {
    if (!la_size_ok(Q, N, L) || !lr_stages_ok(n_stages) || Q == 0 || N == 0) return 0;
    return lr_workspace(Q, N, L, n_stages);
}

int sgpr_landmark_relocalize(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_lm_center,
                             const int32_t* d_lm_label, const uint8_t* d_lm_use, int L, const double* h_radius_in,
                             const double* h_radii, int n_stages, int n_labels, double tau_z, double tau_edge,
                             double min_base, double max_base, int max_hyp, int min_inliers, double sep, int iters,
                             int min_nodes, double* d_poses_out, double* d_coarse, double* d_other,
                             int32_t* d_node_landmark, int32_t* d_stat, int32_t* d_win, int64_t* d_hyp, double* d_rms,
                             int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_relocalize";
    if (!no_negative(fn, {{"Q", Q}, {"N", N}, {"L", L}, {"iters", iters}})) return SGPR_E_INVALID;
    if (!lr_stages_ok(n_stages)) {
        set_error(fn + ": n_stages " + std::to_string(n_stages) + " outside [0, " + std::to_string(SGPR_RELOC_MAX_STAGES) + "]");
        return SGPR_E_INVALID;
    }
    if (!landmark_labels_ok(fn, h_radius_in, n_labels, "h_radius_in")) return SGPR_E_INVALID;
    if (!h_radii && n_stages > 0) {
        set_error(fn + ": NULL h_radii with n_stages " + std::to_string(n_stages));
        return SGPR_E_INVALID;
    }
    if (!radii_ok(fn, h_radius_in, n_labels, "inlier radius")) return SGPR_E_INVALID;
    for (int j = 0; j < n_stages; ++j)
        if (!radii_ok(fn, h_radii + (size_t)j * n_labels, n_labels, "radius", j)) return SGPR_E_INVALID;
    if (!not_negative(fn, "tau_z", tau_z)) return SGPR_E_INVALID;
    if (!not_negative(fn, "tau_edge", tau_edge)) return SGPR_E_INVALID;
    if (!not_negative(fn, "min_base", min_base)) return SGPR_E_INVALID;
    if (!(max_base >= min_base) || !std::isfinite(max_base)) {
        set_error(fn + ": max_base is below min_base or not finite");
        return SGPR_E_INVALID;
    }
    if (max_hyp < 1) {
        set_error(fn + ": max_hyp " + std::to_string(max_hyp) + " is below 1");
        return SGPR_E_INVALID;
    }
    if (min_inliers < 2) {
        set_error(fn + ": min_inliers " + std::to_string(min_inliers) + " is below 2");
        return SGPR_E_INVALID;
    }
    if (min_nodes < 2) {
        set_error(fn + ": min_nodes " + std::to_string(min_nodes) + " is below 2");
        return SGPR_E_INVALID;
    }
    if (!not_negative(fn, "sep", sep)) return SGPR_E_INVALID;
    if (!la_size_ok(Q, N, L)) {
        set_error(fn + ": Q N = " + std::to_string((long long)Q * N) + " exceeds the int32 node index");
        return SGPR_E_INVALID;
    }
    if (Q == 0 || N == 0) return SGPR_OK;
    if (!d_centers || !d_labels || ((!d_lm_center || !d_lm_label) && L > 0) || !d_poses_out || !d_coarse || !d_other ||
        !d_node_landmark || !d_stat || !d_win || !d_hyp || !d_rms || !d_num || !d_workspace) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = lr_workspace(Q, N, L, n_stages);
    if (!workspace_ok(fn, workspace_bytes, need)) return SGPR_E_INVALID;

    Carver ws{static_cast<unsigned char*>(d_workspace)};
    LrArgs a = {};
    a.centers = d_centers;
    a.labels = d_labels;
    a.m = LaMap{d_lm_center, d_lm_label, d_lm_use, L, n_labels, tau_z};
    a.t_in = la_table_carve(ws, (size_t)L);
    a.pair = la_table_carve(ws, (size_t)L);
    for (int j = 0; j < n_stages; ++j) a.t[j] = la_table_carve(ws, (size_t)L);
    int* lab_count = ws.take<int>(2 * LR_LABELS);
    double* stage_radius = ws.take<double>((size_t)n_stages * LR_LABELS);
    a.list = a.pair.elab;
    a.lab_count = lab_count;
    a.stage_radius = stage_radius;
    a.live = N > LR_LDS_SLOTS ? ws.take<int>((size_t)Q * (size_t)N) : nullptr;
    a.poses_out = d_poses_out;
    a.coarse = d_coarse;
    a.other = d_other;
    a.node_landmark = d_node_landmark;
    a.stat = d_stat;
    a.win = d_win;
    a.hyp = reinterpret_cast<long long*>(d_hyp);
    a.rms = d_rms;
    a.num = d_num;
    a.Q = Q;
    a.N = N;
    a.n_stages = n_stages;
    a.max_hyp = max_hyp;
    a.min_inliers = min_inliers;
    a.iters = iters;
    a.min_nodes = min_nodes;
    a.tau_edge = tau_edge;
    a.min_base = min_base;
    a.max_base = max_base;
    a.sep2 = sep * sep;
    a.pair_r = max_base + tau_edge;
    for (int l = 0; l < n_labels; ++l) a.radius_in[l] = h_radius_in[l];

    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(d_num, 0, 4 * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(lab_count, 0, 2 * LR_LABELS * sizeof(int), s);
    // cell_key | cell_head of every table: empty keys, list ends (-1)
    if (e == hipSuccess) e = hipMemsetAsync(a.t_in.g.cell_key, 0xff, grid_clear_bytes((size_t)L), s);
    if (e == hipSuccess) e = hipMemsetAsync(a.pair.g.cell_key, 0xff, grid_clear_bytes((size_t)L), s);
    for (int j = 0; j < n_stages && e == hipSuccess; ++j) e = hipMemsetAsync(a.t[j].g.cell_key, 0xff, grid_clear_bytes((size_t)L), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_relocalize: memset");

    const dim3 block(LR_THREADS);
    const int prep_threads = L > n_labels ? L : n_labels;
    const dim3 prep_grid((prep_threads + LR_THREADS - 1) / LR_THREADS);
    for (int j = -1; j < n_stages; ++j) {
        if (j < 0 && L == 0) continue;                          // (nothing to enter; the stages still carry their radii)
        LrPrepArgs p = {};
        p.m = a.m;
        p.t = j < 0 ? a.t_in : a.t[j];
        p.pair = a.pair;
        p.lab_count = lab_count;
        p.radius_out = j < 0 ? nullptr : stage_radius + (size_t)j * LR_LABELS;
        p.pair_r = a.pair_r;
        p.with_pair = j < 0 ? 1 : 0;
        for (int l = 0; l < n_labels; ++l) p.radius[l] = j < 0 ? h_radius_in[l] : h_radii[(size_t)j * n_labels + l];
        hipLaunchKernelGGL(lr_prep_kernel, prep_grid, block, 0, s, p);
    }
    if (L > 0)
        hipLaunchKernelGGL(lr_list_kernel, dim3((L + LR_THREADS - 1) / LR_THREADS), block, 0, s, a.t_in.elab, L, lab_count,
                           a.pair.elab);
    if (N <= LR_LDS_SLOTS)
        hipLaunchKernelGGL((lr_reloc_kernel<true>), dim3(Q), block, 0, s, a);
    else
        hipLaunchKernelGGL((lr_reloc_kernel<false>), dim3(Q), block, 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_relocalize: launch");
    return SGPR_OK;
}

}  // extern "C"
