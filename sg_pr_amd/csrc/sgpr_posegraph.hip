// Planar pose-graph relaxation over accepted loop closures (sgpr_posegraph_optimize; include/sgpr_posegraph.h,
// DESIGN.md §25): a two-stage linear solve, rotations then translations, each a preconditioned conjugate-gradient
// solve in float64 whose every operation is the header's, so the result is reproducible bit for bit
// (tests/posegraph_ref.py).
//
//   pg_solve_kernel   ONE persistent workgroup of 1024 threads per call.  It prepares the problem (status, the edge
//                     quantities, which sessions are reachable from an anchor, every scan's closure lists in ascending
//                     order), runs stage R and stage T and writes the outputs; it loops on the device and leaves when
//                     converged, so the call needs no host synchronisation and no workgroup ever waits for another.
//
// Inside an iteration a thread owns the scans k = tid, tid + 1024, ... (the operator, the vector updates) and a lane owns
// the segments seg = tid, tid + 1024, ... of the block-tridiagonal preconditioner: 64 dependent steps down and 64 up on
// l, piv and y stored position-major ([position][segment]), so the lanes of a wave read consecutive addresses.  The
// two sums of an iteration follow S literally: a wave reduces a chunk of 1024 (16 strided values per lane are the tree's
// levels h = 512 .. 64, shuffles the levels 32 .. 1), wave 0 reduces the chunk sums.
//
// Integer atomics only (closure counts, the 64 adjacency words, flags); the order they land in decides nothing: every
// closure list is sorted afterwards.  Plain vector stores; contraction is off for the whole file.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_map.hpp"
#include "sgpr_posegraph.h"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int PG_T = 1024;
constexpr int PG_WAVES = PG_T / 64;
constexpr int PG_SEG = SGPR_POSEGRAPH_SEGMENT;
constexpr int PG_CHUNK = 1024;

struct c64 {
    double r, i;
};

__device__ __forceinline__ c64 cmul(const c64& a, const c64& b) { return c64{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
__device__ __forceinline__ c64 cmulc(const c64& a, const c64& v) { return c64{a.r * v.r + a.i * v.i, a.r * v.i - a.i * v.r}; }

// the arguments and the carved workspace; starts[n] = M closes the session table, segbase[s] = segments of sessions < s
struct PgArgs {
    const double* X;
    const int32_t *rows, *cols;
    const double *T, *weight;
    const uint8_t* fixed;
    double* X_out;
    int32_t* info;
    double* resid;
    int M, C, n_sessions, n_seg, max_iters;
    double w_odo[2], w_clo[2], rel_tol;
    int32_t starts[SGPR_SESSION_MAX + 1], segbase[SGPR_SESSION_MAX + 1];
    // per scan
    c64 *g, *t, *r, *p, *Ap, *zv, *ozr, *ozt;
    double* diag;
    int32_t *pos, *slot, *cntH, *cntT, *offH, *offT;
    uint8_t* free;
    // per closure
    c64 *czr, *czt;
    double *cwr, *cwt;
    int32_t *listH, *listT;
    uint8_t* live;
    // position-major [PG_SEG][n_seg]
    c64 *Y, *L;
    double* PIV;
    uint8_t* CPL;
};

size_t pg_segment_cap(int M) { return (size_t)(M / PG_SEG + SGPR_SESSION_MAX); }

size_t pg_ws_bytes(int M, int C) { return 8192 + (size_t)192 * M + (size_t)64 * C + 2624 * pg_segment_cap(M); }

// carve the workspace (every array 256-byte aligned from the base); returns the bytes used
size_t pg_carve(PgArgs& a, void* ws) {
    unsigned char* base = static_cast<unsigned char*>(ws);
    Carver c{base};
    const size_t M = a.M, C = a.C, NS = pg_segment_cap(a.M) * PG_SEG;
    for (c64** v : {&a.g, &a.t, &a.r, &a.p, &a.Ap, &a.zv, &a.ozr, &a.ozt}) *v = c.take<c64>(M);
    a.diag = c.take<double>(M);
    for (int32_t** v : {&a.pos, &a.slot, &a.cntH, &a.cntT}) *v = c.take<int32_t>(M);
    for (int32_t** v : {&a.offH, &a.offT}) *v = c.take<int32_t>(M + 1);
    a.free = c.take<uint8_t>(M);
    for (c64** v : {&a.czr, &a.czt}) *v = c.take<c64>(C);
    for (double** v : {&a.cwr, &a.cwt}) *v = c.take<double>(C);
    for (int32_t** v : {&a.listH, &a.listT}) *v = c.take<int32_t>(C);
    a.live = c.take<uint8_t>(C);
    a.Y = c.take<c64>(NS);
    a.L = c.take<c64>(NS);
    a.PIV = c.take<double>(NS);
    a.CPL = c.take<uint8_t>(NS);
    return (size_t)(c.p - base);
}

// ascending heap sort of n distinct ints (a closure list; usually a handful)
__device__ void pg_sort(int32_t* v, int n) {
    auto sift = [&](int root, int end) {
        for (;;) {
            int child = 2 * root + 1;
            if (child >= end) return;
            if (child + 1 < end && v[child + 1] > v[child]) ++child;
            if (v[root] >= v[child]) return;
            const int32_t x = v[root];
            v[root] = v[child];
            v[child] = x;
            root = child;
        }
    };
    for (int i = n / 2 - 1; i >= 0; --i) sift(i, n);
    for (int end = n - 1; end > 0; --end) {
        const int32_t x = v[0];
        v[0] = v[end];
        v[end] = x;
        sift(0, end);
    }
}

// the running sum of a scan's terms, "starting from the first term"
struct PgAcc {
    double r = 0.0, i = 0.0;
    bool first = true;
    __device__ __forceinline__ void add(double tr, double ti) {
        if (first) {
            r = tr;
            i = ti;
            first = false;
        } else {
            r = r + tr;
            i = i + ti;
        }
    }
};

// the terms of scan k in the order of the definition: f(is_tail, other scan, zr, zt, w_rot, w_trans)
template <class F>
__device__ __forceinline__ void pg_walk(const PgArgs& a, int k, F&& f) {
    if (a.pos[k] > 0) f(false, k - 1, a.ozr[k], a.ozt[k], a.w_odo[0], a.w_odo[1]);
    for (int q = a.offH[k]; q < a.offH[k + 1]; ++q) {
        const int p = a.listH[q];
        f(false, a.cols[p], a.czr[p], a.czt[p], a.cwr[p], a.cwt[p]);
    }
    if (k + 1 < a.M && a.pos[k + 1] > 0) f(true, k + 1, a.ozr[k + 1], a.ozt[k + 1], a.w_odo[0], a.w_odo[1]);
    for (int q = a.offT[k]; q < a.offT[k + 1]; ++q) {
        const int p = a.listT[q];
        f(true, a.rows[p], a.czr[p], a.czt[p], a.cwr[p], a.cwt[p]);
    }
}

// (A x)_k of a free scan
template <bool ROT>
__device__ __forceinline__ c64 pg_apply(const PgArgs& a, const c64* __restrict__ x, int k) {
    PgAcc acc;
    const c64 xk = x[k];
    pg_walk(a, k, [&](bool tail, int o, const c64& z, const c64&, double wr, double wt) {
        const c64 xo = x[o];
        if (ROT) {
            if (!tail) {
                const c64 pr = cmul(z, xo);
                acc.add(wr * (xk.r - pr.r), wr * (xk.i - pr.i));
            } else {
                const c64 pr = cmul(z, xk);
                const c64 d = {wr * (xo.r - pr.r), wr * (xo.i - pr.i)};
                const c64 c = cmulc(z, d);
                acc.add(-c.r, -c.i);
            }
        } else {
            if (!tail)
                acc.add(wt * (xk.r - xo.r), wt * (xk.i - xo.i));
            else
                acc.add(-(wt * (xo.r - xk.r)), -(wt * (xo.i - xk.i)));
        }
    });
    return c64{acc.r, acc.i};
}

// S(a_r b_r + a_i b_i) over the M scans; every thread returns the same double
__device__ double pg_dot(const c64* __restrict__ x, const c64* __restrict__ y, int M, double* csum, double* bcast) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = (M + PG_CHUNK - 1) / PG_CHUNK;
    for (int ch = wave; ch < nch; ch += PG_WAVES) {
        double d[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int k = ch * PG_CHUNK + m * 64 + lane;
            d[m] = 0.0;
            if (k < M) {
                const c64 u = x[k], v = y[k];
                d[m] = u.r * v.r + u.i * v.i;
            }
        }
#pragma unroll
        for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
            for (int m = 0; m < h; ++m) d[m] = d[m] + d[m + h];
        double v = d[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
        if (lane == 0) csum[ch] = v;
    }
    __syncthreads();
    if (wave == 0) {
        int P = 1;
        while (P < nch) P <<= 1;
        double v = lane < nch ? csum[lane] : 0.0;
        for (int off = P >> 1; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
        if (lane == 0) *bcast = v;
    }
    __syncthreads();
    return *bcast;
}

// where segment seg starts and how many scans it holds
__device__ __forceinline__ void pg_segment(const PgArgs& a, int seg, int* k0, int* len) {
    int s = 0;
    for (int j = 1; j < a.n_sessions; ++j) s = a.segbase[j] <= seg ? j : s;
    *k0 = a.starts[s] + (seg - a.segbase[s]) * PG_SEG;
    *len = min(PG_SEG, a.starts[s + 1] - *k0);
}

// zv = M^-1 r: Y holds r position-major on entry; on exit zv holds the result in scan order (a workgroup-wide step)
__device__ void pg_precondition(const PgArgs& a) {
    const int NS = a.n_seg;
    for (int seg = threadIdx.x; seg < NS; seg += PG_T) {
        int k0, len;
        pg_segment(a, seg, &k0, &len);
        c64 prev = {0.0, 0.0};
        for (int j = 0; j < len; ++j) {
            const size_t idx = (size_t)j * NS + seg;
            c64 y = a.Y[idx];
            if (a.CPL[idx]) {
                const c64 pr = cmul(a.L[idx], prev);
                y.r = y.r - pr.r;
                y.i = y.i - pr.i;
                a.Y[idx] = y;
            }
            prev = y;
        }
        for (int j = len - 1; j >= 0; --j) {
            const size_t idx = (size_t)j * NS + seg;
            c64 y = a.Y[idx];
            const double piv = a.PIV[idx];
            y.r = y.r / piv;
            y.i = y.i / piv;
            if (j + 1 < len && a.CPL[idx + NS]) {
                const c64 pr = cmulc(a.L[idx + NS], prev);
                y.r = y.r - pr.r;
                y.i = y.i - pr.i;
            }
            a.Y[idx] = y;
            prev = y;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < a.M; k += PG_T) a.zv[k] = a.free[k] ? a.Y[a.slot[k]] : c64{0.0, 0.0};
    __syncthreads();
}

struct PgShared {
    double csum[64];
    double bcast;
    unsigned long long adj[SGPR_SESSION_MAX];
    unsigned long long anchored, active;
    int status, live, nfree;
    int scanH[PG_T], scanT[PG_T];
};

// one stage: u (holding u0) -> the solution; it / reason / rz0 / rz through out[0..3]
template <bool ROT>
__device__ void pg_stage(const PgArgs& a, c64* u, PgShared& sh, int* iters, int* reason, double* rz0_out,
                         double* rz_out) {
    const int M = a.M, NS = a.n_seg, tid = threadIdx.x;
    const double w_odo = ROT ? a.w_odo[0] : a.w_odo[1];
    // b, diag, r = b - A u (scan order and position-major)
    for (int k = tid; k < M; k += PG_T) {
        c64 b = {0.0, 0.0}, r = {0.0, 0.0};
        double dg = 0.0;
        if (a.free[k]) {
            PgAcc accd;
            PgAcc accb;
            pg_walk(a, k, [&](bool tail, int o, const c64&, const c64& zt, double wr, double wt) {
                accd.add(ROT ? wr : wt, 0.0);
                if (!ROT) {
                    const c64 pr = cmul(a.g[tail ? k : o], zt);
                    if (!tail)
                        accb.add(wt * pr.r, wt * pr.i);
                    else
                        accb.add(-(wt * pr.r), -(wt * pr.i));
                }
            });
            dg = accd.r;
            if (!ROT) b = c64{accb.r, accb.i};
            const c64 au = pg_apply<ROT>(a, u, k);
            r = c64{b.r - au.r, b.i - au.i};
        }
        a.diag[k] = dg;
        a.r[k] = r;
        a.Y[a.slot[k]] = r;
    }
    __syncthreads();
    // the factor of every segment
    for (int seg = tid; seg < NS; seg += PG_T) {
        int k0, len;
        pg_segment(a, seg, &k0, &len);
        double prev = 0.0;
        for (int j = 0; j < len; ++j) {
            const int k = k0 + j;
            const size_t idx = (size_t)j * NS + seg;
            const bool cpl = j > 0 && a.free[k] && a.free[k - 1];
            double piv = a.diag[k];
            c64 l = {0.0, 0.0};
            if (cpl) {
                c64 low;
                if (ROT) {
                    const c64 z = a.ozr[k];
                    low = c64{-(w_odo * z.r), -(w_odo * z.i)};
                } else {
                    low = c64{-w_odo, 0.0};
                }
                l = c64{low.r / prev, low.i / prev};
                piv = piv - (l.r * low.r + l.i * low.i);
            }
            a.L[idx] = l;
            a.PIV[idx] = piv;
            a.CPL[idx] = cpl ? 1 : 0;
            prev = piv;
        }
    }
    // (a lane factors the segments it applies: no barrier needed in between)
    pg_precondition(a);
    for (int k = tid; k < M; k += PG_T) a.p[k] = a.zv[k];
    double rz = pg_dot(a.r, a.zv, M, sh.csum, &sh.bcast);     // (its barriers also publish p)
    const double rz0 = rz, tol2 = a.rel_tol * a.rel_tol;
    int it = 0, why = -1;
    while (it < a.max_iters && rz > tol2 * rz0 && rz > 0.0) {
        for (int k = tid; k < M; k += PG_T) a.Ap[k] = a.free[k] ? pg_apply<ROT>(a, a.p, k) : c64{0.0, 0.0};
        __syncthreads();
        const double pAp = pg_dot(a.p, a.Ap, M, sh.csum, &sh.bcast);
        if (!(pAp > 0.0)) {
            why = SGPR_POSEGRAPH_BREAKDOWN;
            break;
        }
        const double alpha = rz / pAp;
        for (int k = tid; k < M; k += PG_T) {
            c64 r = a.r[k];
            if (a.free[k]) {
                const c64 p = a.p[k], ap = a.Ap[k];
                c64 x = u[k];
                x.r = x.r + alpha * p.r;
                x.i = x.i + alpha * p.i;
                u[k] = x;
                r.r = r.r - alpha * ap.r;
                r.i = r.i - alpha * ap.i;
                a.r[k] = r;
            }
            a.Y[a.slot[k]] = r;
        }
        __syncthreads();
        pg_precondition(a);
        const double rzn = pg_dot(a.r, a.zv, M, sh.csum, &sh.bcast);
        const double beta = rzn / rz;
        for (int k = tid; k < M; k += PG_T) {
            if (a.free[k]) {
                const c64 zv = a.zv[k];
                c64 p = a.p[k];
                p.r = zv.r + beta * p.r;
                p.i = zv.i + beta * p.i;
                a.p[k] = p;
            }
        }
        __syncthreads();
        rz = rzn;
        ++it;
    }
    if (why < 0) why = (rz > tol2 * rz0 && rz > 0.0) ? SGPR_POSEGRAPH_STOP_MAX_ITERS : SGPR_POSEGRAPH_CONVERGED;
    *iters = it;
    *reason = why;
    *rz0_out = rz0;
    *rz_out = rz;
    __syncthreads();
}

__device__ void pg_finish_unsolved(const PgArgs& a, int status, int live, int nfree, int nactive) {
    for (int i = threadIdx.x; i < a.M * 4; i += PG_T) a.X_out[i] = a.X[i];
    if (threadIdx.x == 0) {
        a.info[0] = status;
        for (int j = 1; j < 8; ++j) a.info[j] = 0;
        a.info[5] = live;
        a.info[6] = nfree;
        a.info[7] = nactive;
        for (int j = 0; j < 4; ++j) a.resid[j] = 0.0;
    }
}

__global__ __launch_bounds__(PG_T) void pg_solve_kernel(const PgArgs a) {
    __shared__ PgShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.M, C = a.C, NS = a.n_seg;

    if (tid < SGPR_SESSION_MAX) sh.adj[tid] = 0ull;
    if (tid == 0) {
        sh.anchored = 0ull;
        sh.active = 0ull;
        sh.status = 0;
        sh.live = 0;
        sh.nfree = 0;
    }
    __syncthreads();

    // ---- status; the session, position and slot of every scan; the anchored sessions; the odometry edges
    {
        bool bad = false;
        unsigned long long anch = 0ull;
        for (int k = tid; k < M; k += PG_T) {
            const double c = a.X[(size_t)k * 4], s = a.X[(size_t)k * 4 + 1], x = a.X[(size_t)k * 4 + 2],
                         y = a.X[(size_t)k * 4 + 3];
            if (!(isfinite(c) && isfinite(s) && isfinite(x) && isfinite(y)) || c * c + s * s == 0.0) bad = true;
            const int ss = session_of(a.starts, a.n_sessions, k), pos = k - a.starts[ss];
            a.pos[k] = pos;
            a.slot[k] = (pos % PG_SEG) * NS + a.segbase[ss] + pos / PG_SEG;
            a.cntH[k] = 0;
            a.cntT[k] = 0;
            if (a.fixed ? a.fixed[k] != 0 : k == 0) anch |= 1ull << ss;
            a.g[k] = c64{c, s};
            a.t[k] = c64{x, y};
            if (pos > 0) {
                const c64 gp = {a.X[(size_t)(k - 1) * 4], a.X[(size_t)(k - 1) * 4 + 1]};
                const c64 tp = {a.X[(size_t)(k - 1) * 4 + 2], a.X[(size_t)(k - 1) * 4 + 3]};
                const c64 q = cmulc(gp, c64{c, s});
                const double n = sqrt(q.r * q.r + q.i * q.i);
                a.ozr[k] = c64{q.r / n, q.i / n};
                a.ozt[k] = cmulc(gp, c64{x - tp.r, y - tp.i});
            } else {
                a.ozr[k] = c64{1.0, 0.0};
                a.ozt[k] = c64{0.0, 0.0};
            }
        }
        if (bad) atomicOr(&sh.status, SGPR_POSEGRAPH_NONFINITE);
        if (anch) atomicOr(&sh.anchored, anch);
    }
    __syncthreads();
    int status = sh.status | (sh.anchored == 0ull ? SGPR_POSEGRAPH_NO_ANCHOR : 0);
    if (status) {                                                     // (uniform)
        pg_finish_unsolved(a, status, 0, 0, 0);
        return;
    }

    // ---- closures: the live test, the edge quantities, the counts of every scan, session adjacency
    {
        int nlive = 0;
        for (int p = tid; p < C; p += PG_T) {
            const int r = a.rows[p], c = a.cols[p];
            const double tc = a.T[(size_t)p * 4], ts = a.T[(size_t)p * 4 + 1], tx = a.T[(size_t)p * 4 + 2],
                         ty = a.T[(size_t)p * 4 + 3];
            const double wm = a.weight ? a.weight[p] : 1.0;
            const double n2 = tc * tc + ts * ts;
            const bool live = r >= 0 && r < M && c >= 0 && c < M && r != c && isfinite(tc) && isfinite(ts) && isfinite(tx) &&
                              isfinite(ty) && n2 > 0.0 && isfinite(wm) && wm > 0.0;
            a.live[p] = live ? 1 : 0;
            if (!live) continue;
            ++nlive;
            const double n = sqrt(n2);
            a.czr[p] = c64{tc / n, ts / n};
            a.czt[p] = c64{tx, ty};
            a.cwr[p] = a.w_clo[0] * wm;
            a.cwt[p] = a.w_clo[1] * wm;
            atomicAdd(&a.cntH[r], 1);
            atomicAdd(&a.cntT[c], 1);
            const int sr = session_of(a.starts, a.n_sessions, r), sc = session_of(a.starts, a.n_sessions, c);
            atomicOr(&sh.adj[sr], 1ull << sc);
            atomicOr(&sh.adj[sc], 1ull << sr);
        }
        if (nlive) atomicAdd(&sh.live, nlive);
    }
    __syncthreads();

    // ---- sessions reachable from an anchored one (one wave); exclusive scans of the two counts (block sums first)
    const int per = (M + PG_T - 1) / PG_T, k_lo = min(M, tid * per), k_hi = min(M, k_lo + per);
    {
        int sumH = 0, sumT = 0;
        for (int k = k_lo; k < k_hi; ++k) {
            sumH += a.cntH[k];
            sumT += a.cntT[k];
        }
        sh.scanH[tid] = sumH;
        sh.scanT[tid] = sumT;
    }
    __syncthreads();
    if (wave == 2) {
        const unsigned long long mine = sh.adj[lane];
        unsigned long long reach = sh.anchored;
        for (int round = 0; round < SGPR_SESSION_MAX; ++round) {
            unsigned long long grow = ((reach >> lane) & 1ull) ? mine : 0ull;
            for (int off = 32; off > 0; off >>= 1) grow |= __shfl_xor(grow, off);
            if ((reach | grow) == reach) break;                      // (uniform over the wave)
            reach |= grow;
        }
        if (lane == 0) sh.active = reach;
    } else if (tid == 0 || tid == 64) {
        int* s = tid == 0 ? sh.scanH : sh.scanT;
        int run = 0;
        for (int j = 0; j < PG_T; ++j) {
            const int v = s[j];
            s[j] = run;
            run += v;
        }
    }
    __syncthreads();
    const unsigned long long active = sh.active;
    {
        int runH = sh.scanH[tid], runT = sh.scanT[tid], nfree = 0;
        for (int k = k_lo; k < k_hi; ++k) {
            a.offH[k] = runH;
            a.offT[k] = runT;
            runH += a.cntH[k];
            runT += a.cntT[k];
            const bool fixed = a.fixed ? a.fixed[k] != 0 : k == 0;
            const bool fr = ((active >> session_of(a.starts, a.n_sessions, k)) & 1ull) && !fixed;
            a.free[k] = fr ? 1 : 0;
            nfree += fr ? 1 : 0;
        }
        if (k_hi == M && k_lo < M) {          // (the thread that owns the last scan)
            a.offH[M] = runH;
            a.offT[M] = runT;
        }
        if (nfree) atomicAdd(&sh.nfree, nfree);
    }
    __syncthreads();
    const int live = sh.live, nfree = sh.nfree, nactive = __popcll(active);
    if (live == 0) {                                                  // (uniform) nothing ties the odometry down
        pg_finish_unsolved(a, 0, 0, nfree, nactive);
        return;
    }

    // ---- fill the lists (any order), then sort every scan's two lists
    for (int p = tid; p < C; p += PG_T) {
        if (!a.live[p]) continue;
        const int r = a.rows[p], c = a.cols[p];
        a.listH[a.offH[r] + atomicSub(&a.cntH[r], 1) - 1] = p;
        a.listT[a.offT[c] + atomicSub(&a.cntT[c], 1) - 1] = p;
    }
    __syncthreads();
    for (int k = tid; k < M; k += PG_T) {
        pg_sort(a.listH + a.offH[k], a.offH[k + 1] - a.offH[k]);
        pg_sort(a.listT + a.offT[k], a.offT[k + 1] - a.offT[k]);
    }
    __syncthreads();

    // ---- stage R, normalise, stage T
    int itR, whyR, itT, whyT;
    double rz0R, rzR, rz0T, rzT;
    pg_stage<true>(a, a.g, sh, &itR, &whyR, &rz0R, &rzR);
    {
        bool degenerate = false;
        for (int k = tid; k < M; k += PG_T) {
            if (!a.free[k]) continue;
            const c64 g = a.g[k];
            const double n = sqrt(g.r * g.r + g.i * g.i);
            if (isfinite(n) && n > 0.0) {
                a.g[k] = c64{g.r / n, g.i / n};
            } else {
                a.g[k] = c64{a.X[(size_t)k * 4], a.X[(size_t)k * 4 + 1]};
                degenerate = true;
            }
        }
        if (degenerate) atomicOr(&sh.status, SGPR_POSEGRAPH_DEGENERATE);
    }
    __syncthreads();
    pg_stage<false>(a, a.t, sh, &itT, &whyT, &rz0T, &rzT);

    for (int k = tid; k < M; k += PG_T) {
        double* o = a.X_out + (size_t)k * 4;
        if (a.free[k]) {
            const c64 g = a.g[k], t = a.t[k];
            o[0] = g.r;
            o[1] = g.i;
            o[2] = t.r;
            o[3] = t.i;
        } else {
            for (int j = 0; j < 4; ++j) o[j] = a.X[(size_t)k * 4 + j];
        }
    }
    if (tid == 0) {
        a.info[0] = sh.status;
        a.info[1] = itR;
        a.info[2] = itT;
        a.info[3] = whyR;
        a.info[4] = whyT;
        a.info[5] = live;
        a.info[6] = nfree;
        a.info[7] = nactive;
        a.resid[0] = rz0R;
        a.resid[1] = rzR;
        a.resid[2] = rz0T;
        a.resid[3] = rzT;
    }
}

bool pg_counts_ok(int M, int C) {
    return M >= 0 && M <= SGPR_POSEGRAPH_MAX_SCANS && C >= 0 && C <= SGPR_POSEGRAPH_MAX_CLOSURES;
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_posegraph_optimize_workspace_bytes(int M, int C) { return (!pg_counts_ok(M, C) || M == 0) ? 0 : pg_ws_bytes(M, C); }

int sgpr_posegraph_optimize(const double* d_X, int M, const int32_t* h_starts, int n_sessions, const int32_t* d_rows,
                            const int32_t* d_cols, const double* d_T, const double* d_weight, int C,
                            const uint8_t* d_fixed, double w_odo_rot, double w_odo_trans, double w_clo_rot,
                            double w_clo_trans, int max_iters, double rel_tol, double* d_X_out, int32_t* d_info,
                            double* d_resid, void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_posegraph_optimize";
    if (M < 0 || M > SGPR_POSEGRAPH_MAX_SCANS) {
        set_error(fn + ": M " + std::to_string(M) + " outside [0, " + std::to_string(SGPR_POSEGRAPH_MAX_SCANS) + "]");
        return SGPR_E_INVALID;
    }
    if (C < 0 || C > SGPR_POSEGRAPH_MAX_CLOSURES) {
        set_error(fn + ": C " + std::to_string(C) + " outside [0, " + std::to_string(SGPR_POSEGRAPH_MAX_CLOSURES) + "]");
        return SGPR_E_INVALID;
    }
    if (max_iters < 0 || max_iters > SGPR_POSEGRAPH_MAX_ITERS) {
        set_error(fn + ": max_iters " + std::to_string(max_iters) + " outside [0, " +
                  std::to_string(SGPR_POSEGRAPH_MAX_ITERS) + "]");
        return SGPR_E_INVALID;
    }
    if (!session_table_ok(fn.c_str(), "", h_starts, n_sessions, M)) return SGPR_E_INVALID;
    for (double w : {w_odo_rot, w_odo_trans, w_clo_rot, w_clo_trans})
        if (!(w > 0.0) || !std::isfinite(w)) {
            set_error(fn + ": every weight must be finite and positive");
            return SGPR_E_INVALID;
        }
    if (!(rel_tol >= 0.0)) {
        set_error(fn + ": rel_tol is negative or NaN");
        return SGPR_E_INVALID;
    }
    if (M == 0) return SGPR_OK;
    if (!d_X || !d_X_out || !d_info || !d_resid || (C > 0 && (!d_rows || !d_cols || !d_T))) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = pg_ws_bytes(M, C);
    if (!d_workspace || workspace_bytes < need) {
        set_error(fn + ": workspace of " + std::to_string(need) + " bytes required");
        return SGPR_E_WORKSPACE;
    }
    PgArgs a = {};
    a.X = d_X;
    a.rows = d_rows;
    a.cols = d_cols;
    a.T = d_T;
    a.weight = d_weight;
    a.fixed = d_fixed;
    a.X_out = d_X_out;
    a.info = d_info;
    a.resid = d_resid;
    a.M = M;
    a.C = C;
    a.max_iters = max_iters;
    a.w_odo[0] = w_odo_rot;
    a.w_odo[1] = w_odo_trans;
    a.w_clo[0] = w_clo_rot;
    a.w_clo[1] = w_clo_trans;
    a.rel_tol = rel_tol;
    fill_session_table(a.starts, &a.n_sessions, h_starts, n_sessions);
    a.starts[a.n_sessions] = M;
    a.segbase[0] = 0;
    for (int s = 0; s < a.n_sessions; ++s)
        a.segbase[s + 1] = a.segbase[s] + (a.starts[s + 1] - a.starts[s] + PG_SEG - 1) / PG_SEG;
    a.n_seg = a.segbase[a.n_sessions];
    if (pg_carve(a, d_workspace) > need || (size_t)a.n_seg > pg_segment_cap(M)) {
        set_error(fn + ": internal: the workspace formula does not cover the carve");
        return SGPR_E_INVALID;
    }
    hipLaunchKernelGGL(pg_solve_kernel, dim3(1), dim3(PG_T), 0, static_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "pg_solve_kernel launch");
    return SGPR_OK;
}

}  // extern "C"
