// Localise scans in the map (sgpr_localize_scans; include/sgpr_localize.h): the candidates of the last L
// scans of a query's session, carried forward by the query's odometry, are hypotheses of its pose in the map; the answer
// is the mean of the largest set that agrees with one of them.
//
//   loc_kernel<T>   one workgroup of T threads per query, one thread per slot h = l K + k (T >= the smallest power of
//                   two P2 >= L K; T is chosen per launch from L K).  1. P_h goes to LDS, a dead slot as four NaN - a NaN
//                   fails both comparisons of the agreement test, so a dead slot agrees with nothing without a flag to
//                   read.  2. Every thread walks all slots (every lane reads the same LDS address: a broadcast) and
//                   counts its support in a register.  3. The winner is the maximum of the keys
//                   (support << 32) | (0xffffffff - h), distinct integers, reduced by shuffles and then over the waves
//                   through LDS - the same in any order.  4. The supporters' values, +0 elsewhere, go back to LDS and
//                   are summed by the header's halving tree: levels half >= 64 in LDS, the rest by shuffles in wave 0
//                   (lane i takes lane i + half: the same additions).
//
// Every float64 operation of the definition is rounded on its own (contraction is off for the whole file; division and
// sqrt are the correctly rounded ones), so the outputs are reproducible bit for bit (tests/localize_ref.py).  No
// workspace, no atomics, plain vector stores; the session table travels in the launch arguments.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_localize.h"
#include "sgpr_map.hpp"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

struct LocArgs {
    const double* map;
    const int32_t* cols;
    const double* T;
    const uint8_t* accept;
    const double* odo;
    double* pose;
    int32_t* stat;
    double* spread;
    int M, K, L, n_sessions;
    double max_trans, min_cos;
    int32_t starts[SGPR_SESSION_MAX];
};

__device__ __forceinline__ bool loc_agree(const Se2& a, const Se2& b, double min_cos, double tau2) {
    const double dot = a.c * b.c + a.s * b.s;
    const double dx = a.x - b.x, dy = a.y - b.y;
    return dot >= min_cos && dx * dx + dy * dy <= tau2;
}

// S(v) of the header for N vectors at once: v[n] is this thread's entry (tid < T; +0 at and past P2), buf N rows of T
// doubles.  The sums are valid in thread 0.  Ends with every thread past the last read of buf.
template <int T, int N>
__device__ __forceinline__ void loc_tree(double* buf, double (&v)[N], int P2) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int n = 0; n < N; ++n) buf[n * T + tid] = v[n];
    __syncthreads();
    for (int half = P2 >> 1; half >= 64; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int n = 0; n < N; ++n) buf[n * T + tid] = buf[n * T + tid] + buf[n * T + tid + half];
        }
        __syncthreads();
    }
    if (tid < 64) {
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] = buf[n * T + tid];
        for (int half = P2 >= 64 ? 32 : P2 >> 1; half >= 1; half >>= 1) {
#pragma unroll
            for (int n = 0; n < N; ++n) v[n] = v[n] + __shfl_down(v[n], half);
        }
    }
    __syncthreads();
}

template <int T>
__global__ __launch_bounds__(T) void loc_kernel(const LocArgs a) {
    constexpr int WAVES = T / 64;
    __shared__ double smem[4 * T];
    __shared__ unsigned long long wkey[WAVES];
    __shared__ int wlive[WAVES];
    __shared__ double bsum[4];
    double2* cs = reinterpret_cast<double2*>(smem);
    double2* xy = cs + T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x, K = a.K, LK = a.L * K;
    int P2 = 1;
    while (P2 < LK) P2 <<= 1;

    // the first query of i's session: session_of's rule (sgpr_map.hpp), keeping the start and not the index
    int lo = 0;
    for (int j = 1; j < a.n_sessions; ++j) lo = a.starts[j] <= i ? a.starts[j] : lo;
    const int nl = min(a.L, i - lo + 1);         // scans of the window; slots at or past nl K are dead
    const int nslots = nl * K;

    // 1. the hypothesis of this slot
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    Se2 P = {nan, nan, nan, nan};
    bool live = false;
    if (tid < nslots) {
        const int l = tid / K, k = tid - l * K, j = i - l;
        const size_t cand = (size_t)j * K + k;
        const int col = a.cols[cand];
        if (col >= 0 && col < a.M && (a.accept == nullptr || a.accept[cand] != 0)) {
            Se2 h = se2_compose(se2_load(a.map + (size_t)col * 4), se2_load(a.T + cand * 4));
            if (l > 0)
                h = se2_compose(h, se2_compose(se2_inverse(se2_load(a.odo + (size_t)j * 4)), se2_load(a.odo + (size_t)i * 4)));
            live = se2_finite(h);
            if (live) P = h;
        }
    }
    cs[tid] = make_double2(P.c, P.s);
    xy[tid] = make_double2(P.x, P.y);
    __syncthreads();

    // 2. support: the live slots b != this one that agree with it
    const double min_cos = a.min_cos, tau2 = a.max_trans * a.max_trans;
    int support = 1;
    if (live) {
        for (int b = 0; b < nslots; ++b) {
            const double2 bcs = cs[b], bxy = xy[b];
            const Se2 B = {bcs.x, bcs.y, bxy.x, bxy.y};
            support += (b != tid && loc_agree(P, B, min_cos, tau2)) ? 1 : 0;
        }
    }

    // 3. the winner: the maximum of distinct keys (0 = no live slot; a live key has support >= 1)
    unsigned long long best = live ? ((unsigned long long)support << 32) | (0xffffffffu - (unsigned)tid) : 0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    const unsigned long long lb = __ballot(live);
    if (lane == 0) {
        wkey[wave] = best;
        wlive[wave] = __popcll(lb);
    }
    __syncthreads();
    best = 0ull;
    int nlive = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) {
        best = wkey[v] > best ? wkey[v] : best;
        nlive += wlive[v];
    }
    if (best == 0ull) {          // (uniform)
        if (tid == 0) {
            double* p = a.pose + (size_t)i * 4;
            p[0] = p[1] = p[2] = p[3] = nan;
            a.spread[i] = nan;
            int32_t* st = a.stat + (size_t)i * 4;
            st[0] = 0;
            st[1] = 0;
            st[2] = -1;
            st[3] = SGPR_LOCALIZE_NO_HYPOTHESIS;
        }
        return;
    }
    const int win = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    const int nsup = (int)(best >> 32);
    const double2 wcs = cs[win], wxy = xy[win];
    const Se2 W = {wcs.x, wcs.y, wxy.x, wxy.y};
    const bool sup = live && (tid == win || loc_agree(P, W, min_cos, tau2));
    __syncthreads();             // (every read of the hypotheses is done: the tree reuses their LDS)

    // 4. the fused pose
    double v[4] = {sup ? P.c : 0.0, sup ? P.s : 0.0, sup ? P.x : 0.0, sup ? P.y : 0.0};
    loc_tree<T, 4>(smem, v, P2);
    const double n = (double)nsup;
    if (tid == 0) {
        bsum[0] = v[0];
        bsum[1] = v[1];
        bsum[2] = v[2] / n;
        bsum[3] = v[3] / n;
    }
    __syncthreads();
    const double tx = bsum[2], ty = bsum[3];
    const double ex = P.x - tx, ey = P.y - ty;
    double q[1] = {sup ? ex * ex + ey * ey : 0.0};
    loc_tree<T, 1>(smem, q, P2);
    if (tid == 0) {
        const double sc = bsum[0], ss = bsum[1];
        const double nrm = sqrt(sc * sc + ss * ss);
        int flags = 0;
        double gc, gs;
        if (isfinite(nrm) && nrm > 0.0) {
            gc = sc / nrm;
            gs = ss / nrm;
        } else {
            gc = W.c;
            gs = W.s;
            flags = SGPR_LOCALIZE_DEGENERATE;
        }
        double* p = a.pose + (size_t)i * 4;
        p[0] = gc;
        p[1] = gs;
        p[2] = tx;
        p[3] = ty;
        a.spread[i] = sqrt(q[0] / n);
        int32_t* st = a.stat + (size_t)i * 4;
        st[0] = nsup;
        st[1] = nlive;
        st[2] = win;
        st[3] = flags;
    }
}

template <int T>
int loc_launch(const LocArgs& a, int Q, hipStream_t s) {
    hipLaunchKernelGGL(loc_kernel<T>, dim3(Q), dim3(T), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "loc_kernel launch");
    return SGPR_OK;
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

int sgpr_localize_scans(const double* d_map, int M, const int32_t* d_cols, const double* d_T, const uint8_t* d_accept,
                        int Q, int K, const double* d_odo, const int32_t* h_starts, int n_sessions, int L,
                        double max_trans, double min_cos, double* d_pose, int32_t* d_stat, double* d_spread,
                        void* stream) {
    const std::string fn = "sgpr_localize_scans";
    if (Q < 0 || M < 0) {
        set_error(fn + ": " + (Q < 0 ? "Q " + std::to_string(Q) : "M " + std::to_string(M)) + " is negative");
        return SGPR_E_INVALID;
    }
    if (K < 1 || K > SGPR_LOCALIZE_MAX_K) {
        set_error(fn + ": K " + std::to_string(K) + " outside [1, " + std::to_string(SGPR_LOCALIZE_MAX_K) + "]");
        return SGPR_E_INVALID;
    }
    if (L < 1 || L > SGPR_LOCALIZE_MAX_LEN) {
        set_error(fn + ": L " + std::to_string(L) + " outside [1, " + std::to_string(SGPR_LOCALIZE_MAX_LEN) + "]");
        return SGPR_E_INVALID;
    }
    if (!session_table_ok(fn.c_str(), "", h_starts, n_sessions, Q)) return SGPR_E_INVALID;
    if (!(max_trans >= 0.0)) {
        set_error(fn + ": max_trans is negative or NaN");
        return SGPR_E_INVALID;
    }
    if (std::isnan(min_cos)) {
        set_error(fn + ": min_cos is NaN");
        return SGPR_E_INVALID;
    }
    if (Q == 0) return SGPR_OK;
    if (!d_map || !d_cols || !d_T || !d_pose || !d_stat || !d_spread || (L > 1 && !d_odo)) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    LocArgs a = {};
    a.map = d_map;
    a.cols = d_cols;
    a.T = d_T;
    a.accept = d_accept;
    a.odo = d_odo;
    a.pose = d_pose;
    a.stat = d_stat;
    a.spread = d_spread;
    a.M = M;
    a.K = K;
    a.L = L;
    a.max_trans = max_trans;
    a.min_cos = min_cos;
    fill_session_table(a.starts, &a.n_sessions, h_starts, n_sessions);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int slots = L * K;
    if (slots <= 64) return loc_launch<64>(a, Q, s);
    if (slots <= 128) return loc_launch<128>(a, Q, s);
    if (slots <= 256) return loc_launch<256>(a, Q, s);
    return loc_launch<1024>(a, Q, s);
}

}  // extern "C"
