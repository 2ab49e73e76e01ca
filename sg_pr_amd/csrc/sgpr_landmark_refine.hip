// Refine the poses of a map on its own landmarks (sgpr_landmark_refine; include/sgpr_landmark_refine.h):
// T alternations of "every landmark's centre is the mean of its observations" and "every scan is rigidly re-fitted to
// the centres of its nodes' landmarks in closed form".  Float64 with every operation rounded on its own; the sums over a
// landmark and over the map are fixed-point integer atomics (any order, same sums), the sums over one scan are the
// header's W: a lane's slots in ascending order, then a halving tree of shuffles (wave_tree).  The tree, the wave sums,
// the map point, the closed-form fit and the fixed-point constants are sgpr_map_grid.hpp's, shared with
// sgpr_landmark_align_core.hpp.
//
//   rf_accumulate_kernel  step k, one thread per node: the map point under X_k; a used node adds 1 and its two
//                         fixed-point coordinates to its landmark's slots of accumulator set k & 1 (three 64-bit integer
//                         atomics).  Thread 0 also turns (Q, n) of step k-1 into d_cost[k-1] and clears that pair.
//   rf_fit_kernel         step k, one wave per scan, four per workgroup.  Lane j owns the slots j, j + 64, ..: exactly
//                         partial j of W.  Pass 1: the residual of every used node to its centre (summed as integers
//                         across the wave, one uint64 atomic per wave into Q_k, one into n_k) and W(p), W(l); pass 2: the
//                         centred moments ar, ai.  Lane 0 writes X_{k+1}[g] - or, at k == T, copies X_T[g] to the output
//                         and no pass 2 runs.  The workgroups also clear accumulator set (k + 1) & 1, which is idle during
//                         step k and is the next one written.
//   rf_finish_kernel      one workgroup: d_cost[T], d_info.
//
// Poses alternate between two workspace arrays (X_0 is the caller's), so a fit never reads a pose of its own step:
// Jacobi.  Everything is handed from one kernel to the next on one stream; no workgroup waits for another.  No
// floating-point atomics, no inline assembly, plain vector stores.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_refine.h"
#include "sgpr_map_grid.hpp"

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_WAVES = RF_THREADS / 64;
constexpr int RF_FINISH_THREADS = 1024;
constexpr int RF_SCALARS = 32;                 // uint64 words: Q[2], n[2], re-fitted, kept (the rest pads to 256 bytes)

enum { RF_Q = 0, RF_N = 2, RF_REFIT = 4, RF_KEPT = 5 };
enum { RF_MODE_FIT = 0, RF_MODE_LAST_FIT = 1, RF_MODE_COPY = 2 };

typedef unsigned long long u64;

struct RfArgs {
    const float* centers;
    const int32_t* node_landmark;
    const unsigned char* lm_use;
    const unsigned char* fixed;
    int G, N, L, P, min_nodes;
};

__device__ __forceinline__ Se2 rf_load_pose(const double* X, int g) {
    const double* p = X + 4 * (size_t)g;
    return Se2{p[0], p[1], p[2], p[3]};
}

// node p of a scan with pose X (pose_ok: its doubles are finite): used or not; its widened (x, y), its map point, its id
__device__ __forceinline__ bool rf_node(const RfArgs& a, const Se2& X, bool pose_ok, int p, double& x, double& y,
                                        double& mx, double& my, int& id) {
    id = a.node_landmark[p];
    bool used = pose_ok && id >= 0 && id < a.L;
    used = used && a.lm_use[id] != 0;
    x = (double)a.centers[3 * (size_t)p];
    y = (double)a.centers[3 * (size_t)p + 1];
    se2_apply(X, x, y, &mx, &my);
    return used && in_limit37(mx) && in_limit37(my);
}

__device__ __forceinline__ double rf_cost(u64 q, u64 n) {
    return n == 0 ? __longlong_as_double(0x7ff8000000000000ll) : sqrt((double)q / ((double)n * MAP_FIX));
}

__global__ __launch_bounds__(RF_THREADS) void rf_accumulate_kernel(const RfArgs a, const double* X, u64* acc, u64* scal,
                                                                   double* cost_prev, int prev_slot) {
    const int p = blockIdx.x * RF_THREADS + threadIdx.x;
    if (p == 0 && cost_prev) {                                  // (Q, n) of the step before: final since its fit ended
        *cost_prev = rf_cost(scal[RF_Q + prev_slot], scal[RF_N + prev_slot]);
        scal[RF_Q + prev_slot] = 0ull;
        scal[RF_N + prev_slot] = 0ull;
    }
    if (p >= a.P) return;
    const Se2 Xg = rf_load_pose(X, p / a.N);
    double x, y, mx, my;
    int id;
    if (!rf_node(a, Xg, se2_finite(Xg), p, x, y, mx, my, id)) return;
    atomicAdd(&acc[3 * (size_t)id], 1ull);
    atomicAdd(&acc[3 * (size_t)id + 1], (u64)llrint(mx * MAP_FIX));
    atomicAdd(&acc[3 * (size_t)id + 2], (u64)llrint(my * MAP_FIX));
}

__global__ __launch_bounds__(RF_THREADS) void rf_fit_kernel(const RfArgs a, const double* X, double* X_next,
                                                            const u64* acc, u64* idle, u64* scal, int slot, int mode) {
    if (idle)
        for (size_t i = (size_t)blockIdx.x * RF_THREADS + threadIdx.x; i < 3 * (size_t)a.L; i += (size_t)gridDim.x * RF_THREADS)
            idle[i] = 0ull;
    const int g = blockIdx.x * RF_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= a.G) return;                                       // (whole waves leave: the shuffles below are wave-wide)
    const Se2 Xg = rf_load_pose(X, g);
    const bool pose_ok = se2_finite(Xg);
    const int base = g * a.N;

    double spx = 0.0, spy = 0.0, slx = 0.0, sly = 0.0;
    u64 q = 0ull, cnt = 0ull;
    for (int n = lane; n < a.N; n += 64) {
        double x, y, mx, my;
        int id;
        if (!rf_node(a, Xg, pose_ok, base + n, x, y, mx, my, id)) continue;
        const double den = (double)acc[3 * (size_t)id] * MAP_FIX;
        const double lx = (double)(long long)acc[3 * (size_t)id + 1] / den, ly = (double)(long long)acc[3 * (size_t)id + 2] / den;
        const double ex = mx - lx, ey = my - ly;
        const double d2 = ex * ex + ey * ey;
        q += (u64)llrint(fmin(d2, MAP_D2_CAP) * MAP_FIX);
        cnt += 1ull;
        spx += x;
        spy += y;
        slx += lx;
        sly += ly;
    }
    q = wave_sum(q);
    const int ng = (int)wave_sum(cnt);
    if (lane == 0 && ng > 0) {
        atomicAdd(&scal[RF_Q + slot], q);
        atomicAdd(&scal[RF_N + slot], (u64)ng);
    }
    if (mode == RF_MODE_COPY) {
        if (lane == 0) {
            double* o = X_next + 4 * (size_t)g;
            o[0] = Xg.c;
            o[1] = Xg.s;
            o[2] = Xg.x;
            o[3] = Xg.y;
        }
        return;
    }
    const double dn = (double)ng;
    const double pbx = wave_tree(spx) / dn, pby = wave_tree(spy) / dn, lbx = wave_tree(slx) / dn, lby = wave_tree(sly) / dn;

    double ar = 0.0, ai = 0.0;
    for (int n = lane; n < a.N; n += 64) {
        double x, y, mx, my;
        int id;
        if (!rf_node(a, Xg, pose_ok, base + n, x, y, mx, my, id)) continue;
        const double den = (double)acc[3 * (size_t)id] * MAP_FIX;
        const double lx = (double)(long long)acc[3 * (size_t)id + 1] / den, ly = (double)(long long)acc[3 * (size_t)id + 2] / den;
        const double px = x - pbx, py = y - pby, qx = lx - lbx, qy = ly - lby;
        ar += px * qx + py * qy;
        ai += px * qy - py * qx;
    }
    ar = wave_tree(ar);
    ai = wave_tree(ai);
    const Se2Fit fit = se2_fit(pbx, pby, lbx, lby, ar, ai);
    if (lane != 0) return;
    const bool fixed = a.fixed && a.fixed[g] != 0;
    const bool keep = fixed || ng < a.min_nodes || fit.degenerate();
    const Se2 R = keep ? Xg : fit.F;
    double* o = X_next + 4 * (size_t)g;
    o[0] = R.c;
    o[1] = R.s;
    o[2] = R.x;
    o[3] = R.y;
    if (mode == RF_MODE_LAST_FIT) {
        if (!keep) atomicAdd(&scal[RF_REFIT], 1ull);
        else if (!fixed) atomicAdd(&scal[RF_KEPT], 1ull);
    }
}

__global__ __launch_bounds__(RF_FINISH_THREADS) void rf_finish_kernel(const u64* acc, const u64* scal, int L, int slot,
                                                                      double* cost, int32_t* info) {
    __shared__ int wsum[RF_FINISH_THREADS / 64];
    int seen = 0;
    for (int i = threadIdx.x; i < L; i += RF_FINISH_THREADS) seen += acc[3 * (size_t)i] != 0ull ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) seen += __shfl_down(seen, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = seen;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int total = 0;
    for (int i = 0; i < RF_FINISH_THREADS / 64; ++i) total += wsum[i];
    *cost = rf_cost(scal[RF_Q + slot], scal[RF_N + slot]);
    info[0] = (int32_t)scal[RF_N + slot];
    info[1] = total;
    info[2] = (int32_t)scal[RF_REFIT];
    info[3] = (int32_t)scal[RF_KEPT];
}

bool rf_size_ok(int G, int N, int L) { return G >= 0 && N >= 0 && L >= 0 && (long long)G * (long long)N <= 0x7fffffffll; }

size_t rf_acc_bytes(size_t L) { return align256(2 * 3 * L * sizeof(u64)); }

size_t rf_ws_bytes(size_t G, size_t L) {
    return rf_acc_bytes(L) + align256(RF_SCALARS * sizeof(u64)) + 2 * align256(G * 4 * sizeof(double));
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_refine_workspace_bytes(int G, int N, int L) {
    if (!rf_size_ok(G, N, L) || G == 0 || N == 0) return 0;
    return rf_ws_bytes((size_t)G, (size_t)L);
}

int sgpr_landmark_refine(const float* d_centers, int G, int N, const double* d_poses, const int32_t* d_node_landmark,
                         const uint8_t* d_lm_use, int L, const uint8_t* d_fixed, int iters, int min_nodes,
                         double* d_poses_out, double* d_cost, int32_t* d_info, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_refine";
    if (!no_negative(fn, {{"G", G}, {"N", N}, {"L", L}, {"iters", iters}})) return SGPR_E_INVALID;
    if (min_nodes < 2) {
        set_error(fn + ": min_nodes " + std::to_string(min_nodes) + " is below 2");
        return SGPR_E_INVALID;
    }
    if (!rf_size_ok(G, N, L)) {
        set_error(fn + ": G N = " + std::to_string((long long)G * N) + " exceeds the int32 node index");
        return SGPR_E_INVALID;
    }
    if (G == 0 || N == 0) return SGPR_OK;
    if (!d_centers || !d_poses || !d_node_landmark || (!d_lm_use && L > 0) || !d_poses_out || !d_cost || !d_info || !d_workspace) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = rf_ws_bytes((size_t)G, (size_t)L);
    if (!workspace_ok(fn, workspace_bytes, need)) return SGPR_E_INVALID;

    Carver ws{static_cast<unsigned char*>(d_workspace)};
    u64* acc = ws.take<u64>(2 * 3 * (size_t)L);                 // two sets of [L](cnt, S_x, S_y)
    u64* scal = ws.take<u64>(RF_SCALARS);
    double* Xw[2] = {ws.take<double>(4 * (size_t)G), nullptr};
    Xw[1] = ws.take<double>(4 * (size_t)G);

    RfArgs a = {};
    a.centers = d_centers;
    a.node_landmark = d_node_landmark;
    a.lm_use = d_lm_use;
    a.fixed = d_fixed;
    a.G = G;
    a.N = N;
    a.L = L;
    a.P = (int)((size_t)G * (size_t)N);
    a.min_nodes = min_nodes;

    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(acc, 0, rf_acc_bytes((size_t)L) + align256(RF_SCALARS * sizeof(u64)), s);
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_refine: memset");
    const dim3 node_grid((a.P + RF_THREADS - 1) / RF_THREADS), scan_grid((G + RF_WAVES - 1) / RF_WAVES), block(RF_THREADS);
    const int T = iters;
    for (int k = 0; k <= T; ++k) {
        const double* Xk = k == 0 ? d_poses : Xw[k & 1];
        u64* set = acc + (size_t)(k & 1) * 3 * (size_t)L;
        u64* other = acc + (size_t)((k + 1) & 1) * 3 * (size_t)L;
        hipLaunchKernelGGL(rf_accumulate_kernel, node_grid, block, 0, s, a, Xk, set, scal, k > 0 ? d_cost + (k - 1) : nullptr,
                           (k - 1) & 1);
        if (k == T)
            hipLaunchKernelGGL(rf_fit_kernel, scan_grid, block, 0, s, a, Xk, d_poses_out, set, (u64*)nullptr, scal, k & 1,
                               (int)RF_MODE_COPY);
        else
            hipLaunchKernelGGL(rf_fit_kernel, scan_grid, block, 0, s, a, Xk, Xw[(k + 1) & 1], set, other, scal, k & 1,
                               k == T - 1 ? (int)RF_MODE_LAST_FIT : (int)RF_MODE_FIT);
    }
    hipLaunchKernelGGL(rf_finish_kernel, dim3(1), dim3(RF_FINISH_THREADS), 0, s, acc + (size_t)(T & 1) * 3 * (size_t)L, scal, L,
                       T & 1, d_cost + T, d_info);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_refine: launch");
    return SGPR_OK;
}

}  // extern "C"
