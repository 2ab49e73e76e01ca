/*
 * sgpr_landmark_align.h - align scans to a landmark map: nearest-landmark association and closed-form pose fits
 * (libsgpr_hip.so).  A sixth public header in the style of sgpr_landmark_refine.h: the conventions and
 * error codes of sgpr.h hold here, and neither sgpr.h (its 100 functions, SGPR_ABI_VERSION) nor sgpr_posegraph.h (its two
 * functions) nor sgpr_localize.h (its one) nor sgpr_landmarks.h (its two) nor sgpr_landmark_refine.h (its two) is changed
 * by it.
 *
 * sgpr_landmark_align takes the packed node arrays of Q query scans of N slots, one approximate planar pose per scan in
 * the frame of the map, and the landmarks of a map (centre, label and a mask of those that take part: the records of
 * sgpr_landmark_map).  The scans need not be part of the map.  T times, every node is associated with the nearest
 * eligible landmark of its label inside a gate, and the scan is rigidly re-fitted to its matches in closed form - the
 * fit of sgpr_landmark_refine.h.  Every scan is independent of every other: no sum, no decision and no output of one
 * scan depends on another, or on the order of the scans.
 *
 * ARITHMETIC.  Float64, every operation rounded on its own: no fused multiply-add, division and sqrt correctly rounded.
 * The sums over the nodes of a scan are float64 sums W in an order fixed below.  The result is reproducible bit for bit
 * (tests/landmark_align_ref.py is this text in NumPy).
 *
 * X_0 = d_poses[q].  For k = 0 .. T:
 *
 * MAP POINT of node (q, n) under X_k = (c, s, X, Y), with centre (x, y, z) widened from float32:
 *   mx = (c x - s y) + X,   my = (s x + c y) + Y,   mz = z   (as in sgpr_landmarks.h).
 *
 * LIVE node at k: 0 <= label < n_labels and h_radius[label] > 0; the four doubles of X_k are finite; mx, my, mz are finite
 * and at most 2^37 in magnitude.  Every other node is dead.
 *
 * ELIGIBLE landmark: d_lm_use is NULL or d_lm_use[id] != 0; 0 <= d_lm_label[id] < n_labels and h_radius of that label
 * > 0; its three centre doubles are finite and at most 2^37 in magnitude.
 *
 * MATCH of a live node of label l, r = h_radius[l]: among the eligible landmarks of label l with
 *   ex ex + ey ey <= r r   and   |mz - cz| <= tau_z,      ex = mx - cx, ey = my - cy, (cx, cy, cz) the landmark's centre,
 * the right-hand product formed once, the one with the smallest d2 = ex ex + ey ey, ties to the LOWEST id.  There may be
 * none.  Several nodes of one scan may match the same landmark: there is NO one-to-one rule, every node decides alone.
 *
 * STOP.  k == T:  d_poses_out[q] = X_T, bit for bit.  d_node_landmark[q N + n] = the id of the node's match, -2 for a live
 * node without a match, -1 for a dead node.  d_rms[q] = sqrt(W(d2) / double(matched)) over the matched nodes, the planar
 * RMS distance to their landmarks; the quiet NaN 0x7ff8000000000000 when matched == 0.  d_stat[q] = (matched, live, the
 * number of steps that re-fitted the scan, flags), matched and live counted under X_T.  Otherwise
 *
 * FIT of the scan to its matches, with p = the widened (x, y) of its matched nodes, l = the centres of their landmarks:
 *   W(v)   the scan sum: 64 partials start at 0.0; slot n adds v_n into partial n mod 64, in ascending n, slots that are
 *          not matched skipped; the partials are then reduced by the halving tree v[i] += v[i + h], i < h, h = 32, 16, .. 1;
 *          W = v[0]
 *   n_q    the number of matched nodes of the scan
 *   pb = W(p) / double(n_q),  lb = W(l) / double(n_q)   per component
 *   p' = p - pb,  l' = l - lb
 *   ar = W(p'x l'x + p'y l'y),   ai = W(p'x l'y - p'y l'x)      (two products, one sum or difference, per slot)
 *   h  = sqrt(ar ar + ai ai),    c = ar / h,   s = ai / h
 *   X  = lbx - (c pbx - s pby),  Y = lby - (s pbx + c pby)
 * X_{k+1} = (c, s, X, Y) - the rigid motion that minimises the summed squared distance of the matched nodes to their
 * landmarks - unless the scan KEEPS the bits of X_k: n_q < min_nodes, or h is not a positive finite number, or any of
 * c, s, X, Y is not finite.  A step that keeps the pose has the same inputs as the next, so every later step keeps it too
 * and the answer at T is the answer at k (an implementation may stop there); flags bit 1 (KEPT, value 2) is set.
 *
 * NON-FINITE X_0 (any of its four doubles): d_poses_out[q] = d_poses[q] bit for bit, every node of the scan is -1,
 * d_stat[q] = (0, 0, 0, 1) - flags bit 0 (NONFINITE, value 1) - and d_rms[q] is the quiet NaN.
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation; the radii are a HOST array and are copied into the launch.  The results depend on the arguments
 * alone, on any stream: the workspace need not be initialised.  It needs sgpr_landmark_align_workspace_bytes(Q, N, L)
 * bytes, 256-byte aligned (0 when Q N is 0 or an argument is out of range).  d_poses_out may be d_poses; no other output
 * may overlap an input or another output.
 * Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: Q, N, L or iters < 0;
 * min_nodes < 2; n_labels outside 1..SGPR_LANDMARK_MAX_LABELS; a NULL h_radius; a negative or NaN radius (+inf is a
 * radius); a negative or NaN tau_z; Q N > 2^31 - 1; with Q N > 0, a NULL device pointer (d_lm_use may be NULL: every
 * landmark takes part; d_lm_center and d_lm_label may be NULL when L is 0) or a workspace that is too small.  Q == 0 or
 * N == 0 succeeds without touching the device: NOTHING is written then.
 */
#ifndef SGPR_LANDMARK_ALIGN_H
#define SGPR_LANDMARK_ALIGN_H

#include "sgpr.h"
#include "sgpr_landmarks.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t sgpr_landmark_align_workspace_bytes(int Q, int N, int L);

int sgpr_landmark_align(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_poses,
                        const double* d_lm_center, const int32_t* d_lm_label, const uint8_t* d_lm_use, int L,
                        const double* h_radius, int n_labels, double tau_z, int iters, int min_nodes,
                        double* d_poses_out, int32_t* d_node_landmark, int32_t* d_stat, double* d_rms,
                        void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARK_ALIGN_H */
