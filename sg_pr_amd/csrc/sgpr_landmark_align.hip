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
// The cell table is the search of this build: it was the faster at every size measured, from 106 landmarks up (DESIGN.md
// §31 has the timings).  -DSGPR_ALIGN_SEARCH=2 builds the form that tests every landmark instead - the variant those
// timings are against; it gives the same bits.  No floating-point atomics, no inline assembly, plain vector stores; no
// workgroup waits for another.
#include <math.h>

#include <cmath>
#include <string>

#include "sgpr_internal.hpp"
#include "sgpr_landmark_align.h"
#include "sgpr_map.hpp"

#ifndef SGPR_ALIGN_SEARCH
#define SGPR_ALIGN_SEARCH 1
#endif

namespace sgpr {

#pragma clang fp contract(off)

namespace {

constexpr int LA_THREADS = 256;
constexpr int LA_WAVES = LA_THREADS / 64;
constexpr double LA_LIMIT = 137438953472.0;    // 2^37
constexpr bool LA_TABLE = SGPR_ALIGN_SEARCH != 2;
enum { LA_NONFINITE = 1, LA_KEPT = 2 };

struct LaArgs {
    const float* centers;
    const int32_t* labels;
    const double* poses;
    const double* lm_center;
    const int32_t* lm_label;
    const unsigned char* lm_use;
    double* poses_out;
    int32_t* node_landmark;
    int32_t* stat;
    double* rms;
    int* elab;                     // [L] label of an eligible landmark, -1 of any other
    unsigned long long* cell_key;  // [H]
    int* cell_head;                // [H]
    int* next;                     // [L] linked list of the landmark's cell
    unsigned long long hmask;      // H - 1 (H a power of two)
    int Q, N, L, n_labels, iters, min_nodes;
    double tau_z;
    double radius[SGPR_LANDMARK_MAX_LABELS];
};

__device__ __forceinline__ bool la_in_limit(double v) { return isfinite(v) && fabs(v) <= LA_LIMIT; }

__global__ __launch_bounds__(LA_THREADS) void la_prep_kernel(const LaArgs a) {
    const int i = blockIdx.x * LA_THREADS + threadIdx.x;
    if (i >= a.L) return;
    const int l = a.lm_label[i];
    bool ok = (!a.lm_use || a.lm_use[i] != 0) && l >= 0 && l < a.n_labels;
    const double r = ok ? a.radius[l] : 0.0;
    const double cx = a.lm_center[3 * (size_t)i], cy = a.lm_center[3 * (size_t)i + 1], cz = a.lm_center[3 * (size_t)i + 2];
    ok = ok && r > 0.0 && la_in_limit(cx) && la_in_limit(cy) && la_in_limit(cz);
    a.elab[i] = ok ? l : -1;
    if (!ok || !LA_TABLE) return;
    const double cw = lm_cell_width(r);
    const unsigned long long slot = table_insert(a.cell_key, a.hmask, lm_cell_key(l, lm_cell_coord(cx, cw), lm_cell_coord(cy, cw)));
    a.next[i] = atomicExch(&a.cell_head[slot], i);
}

// the halving tree of W over the 64 partials of a wave; every lane gets v[0]
__device__ __forceinline__ double la_tree(double v) {
    for (int h = 32; h > 0; h >>= 1) v += __shfl_down(v, h);    // (lanes i < h hold v[i] + v[i + h]; the others are not read)
    return __shfl(v, 0);
}

__device__ __forceinline__ int la_wave_sum(int v) {
    for (int h = 32; h > 0; h >>= 1) v += __shfl_down(v, h);
    return __shfl(v, 0);
}

// the match of a map point of label l: landmark o is better than the best so far when it passes the gate and comes
// first by (d2, id)
struct LaBest {
    int id;
    double d2, cx, cy;
};

__device__ __forceinline__ void la_test(const LaArgs& a, int o, double mx, double my, double mz, double r2, LaBest& b) {
    const double cx = a.lm_center[3 * (size_t)o], cy = a.lm_center[3 * (size_t)o + 1], cz = a.lm_center[3 * (size_t)o + 2];
    const double ex = mx - cx, ey = my - cy;
    const double d2 = ex * ex + ey * ey;
    if (!(d2 <= r2 && fabs(mz - cz) <= a.tau_z)) return;
    if (b.id >= 0 && !(d2 < b.d2 || (d2 == b.d2 && o < b.id))) return;
    b.id = o;
    b.d2 = d2;
    b.cx = cx;
    b.cy = cy;
}

template <bool TABLE>
__device__ __forceinline__ void la_match(const LaArgs& a, int l, double r, double mx, double my, double mz, LaBest& b) {
    const double r2 = r * r;
    if (TABLE) {
        const double cw = lm_cell_width(r);
        const long long ix = lm_cell_coord(mx, cw), iy = lm_cell_coord(my, cw);
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const unsigned long long slot = table_find(a.cell_key, a.hmask, lm_cell_key(l, ix + dx, iy + dy));
                if (slot == TABLE_EMPTY) continue;
                for (int o = a.cell_head[slot]; o >= 0; o = a.next[o])
                    if (a.elab[o] == l) la_test(a, o, mx, my, mz, r2, b);     // (a shared list: see lm_cell_key)
            }
    } else {
        for (int o = 0; o < a.L; ++o)
            if (a.elab[o] == l) la_test(a, o, mx, my, mz, r2, b);
    }
}

template <bool TABLE>
__global__ __launch_bounds__(LA_THREADS) void la_align_kernel(const LaArgs a) {
    const int q = blockIdx.x * LA_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= a.Q) return;                                       // (whole waves leave: the shuffles below are wave-wide)
    const double* xp = a.poses + 4 * (size_t)q;
    Se2 X = Se2{xp[0], xp[1], xp[2], xp[3]};
    const size_t base = (size_t)q * (size_t)a.N;
    const float* cen = a.centers + 3 * base;
    const int32_t* lab = a.labels + base;
    int32_t* row = a.node_landmark + base;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    int matched = 0, live = 0, refits = 0, flags = 0;
    double sd2 = 0.0;
    if (!se2_finite(X)) {
        for (int n = lane; n < a.N; n += 64) row[n] = -1;
        flags = LA_NONFINITE;
    } else {
        for (int k = 0;; ++k) {
            double spx = 0.0, spy = 0.0, slx = 0.0, sly = 0.0;
            int cnt = 0, lv = 0;
            sd2 = 0.0;
            for (int n = lane; n < a.N; n += 64) {
                const int l = lab[n];
                const double x = (double)cen[3 * (size_t)n], y = (double)cen[3 * (size_t)n + 1], mz = (double)cen[3 * (size_t)n + 2];
                const double mx = (X.c * x - X.s * y) + X.x, my = (X.s * x + X.c * y) + X.y;
                bool alive = l >= 0 && l < a.n_labels;
                const double r = alive ? a.radius[l] : 0.0;
                alive = alive && r > 0.0 && la_in_limit(mx) && la_in_limit(my) && la_in_limit(mz);
                LaBest b = {-2, 0.0, 0.0, 0.0};
                if (alive) la_match<TABLE>(a, l, r, mx, my, mz, b);
                row[n] = alive ? b.id : -1;
                lv += alive ? 1 : 0;
                if (!alive || b.id < 0) continue;
                cnt += 1;
                spx += x;
                spy += y;
                slx += b.cx;
                sly += b.cy;
                sd2 += b.d2;
            }
            matched = la_wave_sum(cnt);
            live = la_wave_sum(lv);
            if (k == a.iters) break;
            if (matched < a.min_nodes) {
                flags |= LA_KEPT;
                break;
            }
            const double dn = (double)matched;
            const double pbx = la_tree(spx) / dn, pby = la_tree(spy) / dn, lbx = la_tree(slx) / dn, lby = la_tree(sly) / dn;
            double ar = 0.0, ai = 0.0;
            for (int n = lane; n < a.N; n += 64) {
                const int id = row[n];
                if (id < 0) continue;
                const double x = (double)cen[3 * (size_t)n], y = (double)cen[3 * (size_t)n + 1];
                const double lx = a.lm_center[3 * (size_t)id], ly = a.lm_center[3 * (size_t)id + 1];
                const double px = x - pbx, py = y - pby, qx = lx - lbx, qy = ly - lby;
                ar += px * qx + py * qy;
                ai += px * qy - py * qx;
            }
            ar = la_tree(ar);
            ai = la_tree(ai);
            const double h = sqrt(ar * ar + ai * ai);
            Se2 F;
            F.c = ar / h;
            F.s = ai / h;
            F.x = lbx - (F.c * pbx - F.s * pby);
            F.y = lby - (F.s * pbx + F.c * pby);
            if (!(h > 0.0 && isfinite(h)) || !se2_finite(F)) {      // (the same bits in every lane: a uniform branch)
                flags |= LA_KEPT;
                break;
            }
            X = F;
            ++refits;
        }
    }
    const double total = la_tree(sd2);
    if (lane != 0) return;
    double* o = a.poses_out + 4 * (size_t)q;
    o[0] = X.c;
    o[1] = X.s;
    o[2] = X.x;
    o[3] = X.y;
    a.rms[q] = matched > 0 ? sqrt(total / (double)matched) : qnan;
    int32_t* st = a.stat + 4 * (size_t)q;
    st[0] = matched;
    st[1] = live;
    st[2] = refits;
    st[3] = flags;
}

bool la_size_ok(int Q, int N, int L) { return Q >= 0 && N >= 0 && L >= 0 && (long long)Q * (long long)N <= 0x7fffffffll; }

size_t la_ws_bytes(size_t L) {
    const size_t h = table_slots(L);
    return align256(L * 4) * 2 + align256(h * 8) + align256(h * 4);
}

}  // namespace
}  // namespace sgpr

using namespace sgpr;

extern "C" {

size_t sgpr_landmark_align_workspace_bytes(int Q, int N, int L) {
    if (!la_size_ok(Q, N, L) || Q == 0 || N == 0) return 0;
    return la_ws_bytes((size_t)L);
}

int sgpr_landmark_align(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_poses,
                        const double* d_lm_center, const int32_t* d_lm_label, const uint8_t* d_lm_use, int L,
                        const double* h_radius, int n_labels, double tau_z, int iters, int min_nodes,
                        double* d_poses_out, int32_t* d_node_landmark, int32_t* d_stat, double* d_rms,
                        void* d_workspace, size_t workspace_bytes, void* stream) {
    const std::string fn = "sgpr_landmark_align";
    if (Q < 0 || N < 0 || L < 0 || iters < 0) {
        set_error(fn + ": " + (Q < 0 ? "Q " + std::to_string(Q) : N < 0 ? "N " + std::to_string(N)
                               : L < 0 ? "L " + std::to_string(L) : "iters " + std::to_string(iters)) + " is negative");
        return SGPR_E_INVALID;
    }
    if (min_nodes < 2) {
        set_error(fn + ": min_nodes " + std::to_string(min_nodes) + " is below 2");
        return SGPR_E_INVALID;
    }
    if (n_labels < 1 || n_labels > SGPR_LANDMARK_MAX_LABELS) {
        set_error(fn + ": n_labels " + std::to_string(n_labels) + " outside [1, " + std::to_string(SGPR_LANDMARK_MAX_LABELS) + "]");
        return SGPR_E_INVALID;
    }
    if (!h_radius) {
        set_error(fn + ": NULL h_radius");
        return SGPR_E_INVALID;
    }
    for (int l = 0; l < n_labels; ++l)
        if (!(h_radius[l] >= 0.0)) {
            set_error(fn + ": radius of label " + std::to_string(l) + " is negative or NaN");
            return SGPR_E_INVALID;
        }
    if (!(tau_z >= 0.0)) {
        set_error(fn + ": tau_z is negative or NaN");
        return SGPR_E_INVALID;
    }
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
    const size_t need = la_ws_bytes((size_t)L);
    if (workspace_bytes < need) {
        set_error(fn + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed");
        return SGPR_E_INVALID;
    }

    Carver ws{static_cast<unsigned char*>(d_workspace)};
    const size_t H = table_slots((size_t)L);
    LaArgs a = {};
    a.centers = d_centers;
    a.labels = d_labels;
    a.poses = d_poses;
    a.lm_center = d_lm_center;
    a.lm_label = d_lm_label;
    a.lm_use = d_lm_use;
    a.poses_out = d_poses_out;
    a.node_landmark = d_node_landmark;
    a.stat = d_stat;
    a.rms = d_rms;
    a.elab = ws.take<int>((size_t)L);
    a.next = ws.take<int>((size_t)L);
    a.cell_key = ws.take<unsigned long long>(H);
    a.cell_head = ws.take<int>(H);
    a.hmask = H - 1;
    a.Q = Q;
    a.N = N;
    a.L = L;
    a.n_labels = n_labels;
    a.iters = iters;
    a.min_nodes = min_nodes;
    a.tau_z = tau_z;
    for (int l = 0; l < n_labels; ++l) a.radius[l] = h_radius[l];

    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (LA_TABLE) {
        // cell_key | cell_head: empty keys, list ends (-1)
        const hipError_t e = hipMemsetAsync(a.cell_key, 0xff, align256(H * 8) + align256(H * 4), s);
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
