// Align scans to a landmark map (sgpr_landmark_align; include/sgpr_landmark_align.h): T rounds of "every
// node takes the nearest eligible landmark of its label inside the gate" and "the scan is rigidly re-fitted to its
// matches in closed form".  Float64 with every operation rounded on its own; the scans are independent, so the whole
// iteration of a scan runs in one wave and nothing is summed across scans.  The sums over a scan are the header's W: a
// lane's slots in ascending order, then a halving tree of shuffles.
//
//   la_prep_kernel    one thread per landmark: eligible or not - its label, or -1, into the workspace - and an
//                     eligible landmark enters the open-addressing cell table of sgpr_map.hpp (cell
//                     width, coordinate and key are sgpr_landmarks.hip's) and is pushed on its cell's linked list.  The
//                     order of a list is whatever the atomics make it; the minimum by (d2, id) does not depend on it.
//   la_align_kernel   one wave per scan, four per workgroup, all T + 1 steps in one launch.  Lane j owns the slots j,
//                     j + 64, ..: exactly partial j of W.  Pass 1 of a step: the map point of every slot, its match - the
//                     lists of the 9 cells around it (or, in the variant, every landmark) - parked in the scan's own
//                     row of d_node_landmark (a lane holds ceil(N / 64) slots: too many for registers at any N), and
//                     W(p), W(l), W(d2).  Pass 2: the centred moments ar, ai from the parked ids; a lane reads back only
//                     what it wrote itself.  At k == T, or at the first step that keeps the pose (every later step
//                     would keep it too), the row already holds the answer and lane 0 writes pose, stat and rms.
//
// What a wave does with a scan - the eligible rule, the match, the sums, the fit, the keep rule - is la_prep_landmark and
// la_fit_scan of sgpr_landmark_align_core.hpp, which sgpr_landmark_track.hip runs per scan and stage; the
// kernels here are the launch shapes around them.  The cell grid, the wave sums and the closed-form fit those two are
// made of are sgpr_map_grid.hpp's.
//
// The cell table is the search of this build: it was the faster at every size measured, from 106 landmarks up (DESIGN.md
// §31 has the timings).  -DSGPR_ALIGN_SEARCH=2 builds the form that tests every landmark instead - the variant those
// timings are against; it gives the same bits.  No floating-point atomics, no inline assembly, plain vector stores; no
// workgroup waits for another.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_align.h"
#include "sgpr_landmark_align_core.hpp"
#include "sgpr_map_grid.hpp"

#ifndef SGPR_ALIGN_SEARCH
#define SGPR_ALIGN_SEARCH 1
#endif

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int LA_THREADS = 256;
constexpr int LA_WAVES = LA_THREADS / 64;
constexpr bool LA_TABLE = SGPR_ALIGN_SEARCH != 2;

struct LaArgs {
    const float* centers;
    const int32_t* labels;
    const double* poses;
    LaMap m;
    LaTable t;
    double* poses_out;
    int32_t* node_landmark;
    int32_t* stat;
    double* rms;
    int Q, N, iters, min_nodes;
    double radius[SGPR_LANDMARK_MAX_LABELS];
};

__global__ __launch_bounds__(LA_THREADS) void la_prep_kernel(const LaArgs a) {
    const int i = blockIdx.x * LA_THREADS + threadIdx.x;
    if (i >= a.m.L) return;
    la_prep_landmark<LA_TABLE>(a.m, a.t, a.radius, i);
}

template <bool TABLE>
__global__ __launch_bounds__(LA_THREADS) void la_align_kernel(const LaArgs a) {
    const int q = blockIdx.x * LA_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= a.Q) return;                                       // (whole waves leave: the shuffles below are wave-wide)
    const double* xp = a.poses + 4 * (size_t)q;
    Se2 X = Se2{xp[0], xp[1], xp[2], xp[3]};
    const size_t base = (size_t)q * (size_t)a.N;
    const LaScanGlobal sc = {a.centers + 3 * base, a.labels + base};
    const LaFit f = la_fit_scan<TABLE>(a.m, a.t, a.radius, sc, a.N, lane, a.node_landmark + base, a.iters, a.min_nodes, X);
    const double rms = la_rms(f);
    if (lane != 0) return;
    double* o = a.poses_out + 4 * (size_t)q;
    o[0] = X.c;
    o[1] = X.s;
    o[2] = X.x;
    o[3] = X.y;
    a.rms[q] = rms;
    int32_t* st = a.stat + 4 * (size_t)q;
    st[0] = f.matched;
    st[1] = f.live;
    st[2] = f.refits;
    st[3] = f.flags;
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_align_workspace_bytes(int Q, int N, int L) {
    if (!la_size_ok(Q, N, L) || Q == 0 || N == 0) return 0;
    return la_table_bytes((size_t)L);
}

int sgpr_landmark_align(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_poses,
                        const double* d_lm_center, const int32_t* d_lm_label, const uint8_t* d_lm_use, int L,
                        const double* h_radius, int n_labels, double tau_z, int iters, int min_nodes,
                        double* d_poses_out, int32_t* d_node_landmark, int32_t* d_stat, double* d_rms,
                        void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_align";
    if (!no_negative(fn, {{"Q", Q}, {"N", N}, {"L", L}, {"iters", iters}})) return SGPR_E_INVALID;
    if (min_nodes < 2) {
        set_error(fn + ": min_nodes " + std::to_string(min_nodes) + " is below 2");
        return SGPR_E_INVALID;
    }
    if (!landmark_labels_ok(fn, h_radius, n_labels) || !radii_ok(fn, h_radius, n_labels)) return SGPR_E_INVALID;
    if (!not_negative(fn, "tau_z", tau_z)) return SGPR_E_INVALID;
    if (!la_size_ok(Q, N, L)) {
        set_error(fn + ": Q N = " + std::to_string((long long)Q * N) + " exceeds the int32 node index");
        return SGPR_E_INVALID;
    }
    if (Q == 0 || N == 0) return SGPR_OK;
    if (!d_centers || !d_labels || !d_poses || ((!d_lm_center || !d_lm_label) && L > 0) || !d_poses_out || !d_node_landmark ||
        !d_stat || !d_rms || !d_workspace) {
        set_error(fn + ": NULL argument");
        return SGPR_E_INVALID;
    }
    const size_t need = la_table_bytes((size_t)L);
    if (!workspace_ok(fn, workspace_bytes, need)) return SGPR_E_INVALID;

    Carver ws{static_cast<unsigned char*>(d_workspace)};
    LaArgs a = {};
    a.centers = d_centers;
    a.labels = d_labels;
    a.poses = d_poses;
    a.m = LaMap{d_lm_center, d_lm_label, d_lm_use, L, n_labels, tau_z};
    a.t = la_table_carve(ws, (size_t)L);
    a.poses_out = d_poses_out;
    a.node_landmark = d_node_landmark;
    a.stat = d_stat;
    a.rms = d_rms;
    a.Q = Q;
    a.N = N;
    a.iters = iters;
    a.min_nodes = min_nodes;
    for (int l = 0; l < n_labels; ++l) a.radius[l] = h_radius[l];

    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (LA_TABLE) {
        // cell_key | cell_head: empty keys, list ends (-1)
        const hipError_t e = hipMemsetAsync(a.t.g.cell_key, 0xff, grid_clear_bytes((size_t)L), s);
        if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_align: memset");
    }
    const dim3 block(LA_THREADS), scan_grid((Q + LA_WAVES - 1) / LA_WAVES);
    if (L > 0) hipLaunchKernelGGL(la_prep_kernel, dim3((L + LA_THREADS - 1) / LA_THREADS), block, 0, s, a);
    hipLaunchKernelGGL(la_align_kernel<LA_TABLE>, scan_grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sgpr_landmark_align: launch");
    return SGPR_OK;
}

}  // extern "C"
