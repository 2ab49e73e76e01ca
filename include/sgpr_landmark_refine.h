/*
 * sgpr_landmark_refine.h - refine the poses of a map on its own landmarks: alternating closed-form pose fits
 * (libsgpr_hip.so).  A fifth public header in the style of sgpr_landmarks.h: the conventions and error
 * codes of sgpr.h hold here, and neither sgpr.h (its 100 functions, SGPR_ABI_VERSION) nor sgpr_posegraph.h (its two
 * functions) nor sgpr_localize.h (its one) nor sgpr_landmarks.h (its two) is changed by it.
 *
 * sgpr_landmark_refine takes the packed node centres of G scans of N slots, one planar pose per scan (X_out of
 * sgpr_posegraph_optimize), the landmark of every node (d_node_landmark of sgpr_landmark_map, made on those poses) and a
 * mask of the L landmarks that take part.  It alternates T times: every landmark's centre is the mean of its
 * observations under the current poses, and every scan is rigidly re-fitted to the centres of its nodes' landmarks in
 * closed form.  All scans of one step are fitted against the centres of that step (Jacobi): no pose of step k+1 is read
 * before every pose of step k has been fitted, so the result does not depend on the order of the scans.
 *
 * ARITHMETIC.  Float64, every operation rounded on its own: no fused multiply-add, division and sqrt correctly rounded.
 * Sums over the observations of a landmark and over all nodes are INTEGER sums of fixed-point values and so order-free;
 * the sums over the nodes of ONE scan are float64 sums W in an order fixed below.  The result is reproducible bit for bit
 * (tests/landmark_refine_ref.py is this text in NumPy).
 *
 * X_0 = d_poses.  For k = 0 .. T:
 *
 * MAP POINT of node (g, n) under X_k[g] = (c, s, X, Y), with centre (x, y, .) widened from float32:
 *   mx = (c x - s y) + X,   my = (s x + c y) + Y   (as in sgpr_landmarks.h; z takes no part).
 *
 * USED node at k: its id = d_node_landmark[g N + n] has 0 <= id < L and d_lm_use[id] != 0; the four doubles of X_k[g] are
 * finite; mx and my are finite and at most 2^37 in magnitude.  Every other node takes no part in step k.
 *
 * CENTRES.  Per landmark, over its used nodes: cnt, and the int64 sums S_x, S_y of llrint(m 2^24) (round to nearest
 * even; they wrap modulo 2^64 as the reference's do).  centre = double(S) / (double(cnt) * 16777216.0).
 *
 * COST.  cost[k] = sqrt(double(Q_k) / (double(n_k) * 16777216.0)): Q_k = the uint64 sum over the used nodes of
 * llrint(min(d2, 1048576.0) * 16777216.0), d2 = ex ex + ey ey, ex = mx - centre_x, ey = my - centre_y of the node's own
 * landmark; n_k = the number of used nodes.  The planar RMS distance of the observations to their centres, each capped
 * at 1024 m.  n_k == 0: cost[k] is the quiet NaN 0x7ff8000000000000.
 *
 * STOP.  k == T: X_out = X_T, bit for bit.  Otherwise
 *
 * FIT of scan g against the centres of step k, with p = the widened (x, y) of its used nodes, l = their centres:
 *   W(v)   the scan sum: 64 partials start at 0.0; slot n adds v_n into partial n mod 64, in ascending n, unused slots
 *          skipped; the partials are then reduced by the halving tree v[i] += v[i + h], i < h, h = 32, 16, .. 1; W = v[0]
 *   n_g    the number of used nodes of the scan
 *   pb = W(p) / double(n_g),  lb = W(l) / double(n_g)   per component
 *   p' = p - pb,  l' = l - lb
 *   ar = W(p'x l'x + p'y l'y),   ai = W(p'x l'y - p'y l'x)      (two products, one sum or difference, per slot)
 *   h  = sqrt(ar ar + ai ai),    c = ar / h,   s = ai / h
 *   X  = lbx - (c pbx - s pby),  Y = lby - (s pbx + c pby)
 * X_{k+1}[g] = (c, s, X, Y) - the rigid motion that minimises the summed squared distance of the scan's used nodes to
 * their centres - unless the scan KEEPS the bits of X_k[g]: it is fixed (d_fixed[g] != 0), or n_g < min_nodes, or h is not
 * a positive finite number, or any of c, s, X, Y is not finite.
 *
 * d_cost [T+1] gets cost[0 .. T].  d_info [4] = (n_T, the landmarks with cnt > 0 at T, the scans the last fit re-fitted,
 * the scans that are not fixed and that the last fit kept); the last two are 0 when T == 0.
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation: 2 T + 4 operations on the stream.  The results depend on the arguments alone, on any stream: the
 * workspace need not be initialised.  It needs sgpr_landmark_refine_workspace_bytes(G, N, L) bytes, 256-byte aligned (0
 * when G N is 0 or an argument is out of range).  d_poses_out may be d_poses.
 * Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: G, N, L or iters < 0;
 * min_nodes < 2; G N > 2^31 - 1; with G N > 0, a NULL device pointer (d_fixed may be NULL: no scan is fixed; d_lm_use may
 * be NULL when L is 0) or a workspace that is too small.  G == 0 or N == 0 succeeds without touching the device: NOTHING
 * is written then.
 */
#ifndef SGPR_LANDMARK_REFINE_H
#define SGPR_LANDMARK_REFINE_H

#include "sgpr.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t sgpr_landmark_refine_workspace_bytes(int G, int N, int L);

int sgpr_landmark_refine(const float* d_centers, int G, int N, const double* d_poses, const int32_t* d_node_landmark,
                         const uint8_t* d_lm_use, int L, const uint8_t* d_fixed, int iters, int min_nodes,
                         double* d_poses_out, double* d_cost, int32_t* d_info, void* d_workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARK_REFINE_H */
