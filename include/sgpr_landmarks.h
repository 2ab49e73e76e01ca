/*
 * sgpr_landmarks.h - the semantic landmark map: the nodes of every scan of a map, fused in the map frame
 * (libsgpr_hip.so).  A fourth public header in the style of sgpr_localize.h: the conventions, error codes
 * and SESSION TABLE rules of sgpr.h hold here, and neither sgpr.h (its 100 functions, SGPR_ABI_VERSION) nor
 * sgpr_posegraph.h (its two functions) nor sgpr_localize.h (its one) is changed by it.
 *
 * sgpr_landmark_map takes the packed node arrays of sgpr_embed / sgpr_verify_pairs for G scans of N slots, one planar
 * pose per scan (X_out of sgpr_posegraph_optimize, or the planar ground truth) and a link radius per label.  It puts
 * every node into the map frame, links nodes of one label that lie within that label's radius of one another, and
 * returns the connected components of the link graph as landmarks: position, label, observation count, lowest member,
 * the sessions that saw it, and the RMS distance of its observations to it.
 *
 * ARITHMETIC.  All arithmetic is float64 and every operation is rounded on its own: no fused multiply-add, division and
 * sqrt correctly rounded.  Sums over the members of a landmark are INTEGER sums of fixed-point values, so they - and
 * every output - do not depend on the order of execution.  The result is reproducible bit for bit
 * (tests/landmark_ref.py is this text in NumPy).
 *
 * MAP POINT of node (g, n), flat index p = g N + n, with centre (x, y, z) widened from float32 and pose (c, s, X, Y) =
 * d_poses[g]:   mx = (c x - s y) + X,   my = (s x + c y) + Y,   mz = z.
 *
 * LIVE node: 0 <= label < n_labels and h_radius[label] > 0; the pose's four doubles are finite; mx, my, mz are finite;
 * |mx|, |my| and |mz| are at most 2^37 m (137 million km).  Beyond that limit the node is dead, so that
 * llrint(m 2^24) below always fits 64 bits.  Every other node is dead: it belongs to no landmark and gets
 * d_node_landmark = -1.  (Padding slots carry label -1 and are dead.)
 *
 * LINK.  Two live nodes a, b of the same label l link iff  dx dx + dy dy <= r r  and  |mz_a - mz_b| <= tau_z,  where
 * dx = mx_a - mx_b, dy = my_a - my_b, r = h_radius[l], and the right-hand product is formed once.  The test is symmetric
 * in bits.  Nodes of one scan may link: there is no cannot-link rule.
 *
 * LANDMARK = a connected component of the link graph.  Landmarks are numbered 0 .. L-1 by ascending lowest flat node
 * index of their members; that index is d_lm_first.  d_node_landmark [G,N] holds the id of every live node, even when it
 * is >= max_landmarks.  d_num[0] = L, which may exceed max_landmarks: then only the records of landmarks
 * 0 .. max_landmarks-1 are written - every byte of those, nothing past them.  d_num[1] = the number of live nodes.
 *
 * RECORD of a landmark with members m:
 *   label     the members' label
 *   count     the number of members
 *   sessions  the OR of (1 << session(g)) over the members; session(g) = the largest j with h_starts[j] <= g (0 without
 *             a table)
 *   center[k] = double(S_k) / (double(count) * 16777216.0),  S_k = the int64 sum of llrint(m_k * 16777216.0) over the
 *             members, k = x, y, z (round to nearest even; m_k 2^24 is exact)
 *   spread    = sqrt(double(Q) / (double(count) * 16777216.0)),  Q = the uint64 sum of
 *             llrint(min(d2, 1048576.0) * 16777216.0),  d2 = ex ex + ey ey,  ex = mx - center[0], ey = my - center[1]:
 *             the planar RMS distance of the members to the centre, every distance capped at 1024 m
 * The integer sums wrap modulo 2^64 (two's complement for S_k), as the reference's do.  S_k cannot wrap while
 * count x max|m_k| < 2^39 m (a million observations 500 km from the origin), Q not while count < 2^20 or every member
 * lies within 1 m of its centre x sqrt(2^20 / count); past that the record is still reproducible, and meaningless.
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation; the session table and the radii are HOST arrays and are copied into the launches.  The results depend
 * on the arguments alone, on any stream: the workspace need not be initialised and holds nothing afterwards.  It needs
 * sgpr_landmark_workspace_bytes(G, N) bytes, 256-byte aligned (0 when G N is 0 or out of range).
 * Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: G, N or max_landmarks < 0;
 * n_labels outside 1..SGPR_LANDMARK_MAX_LABELS; a NULL h_radius; a negative or NaN radius (+inf is a radius); a negative
 * or NaN tau_z; a bad session table (of the G scans); G N > 2^31 - 1; with G N > 0, a NULL device pointer (the six
 * record arrays may be NULL when max_landmarks is 0) or a workspace that is too small.  G == 0 or N == 0 succeeds
 * without touching the device: NOTHING is written then, d_num included - the answer is (0, 0) and the caller knows it.
 */
#ifndef SGPR_LANDMARKS_H
#define SGPR_LANDMARKS_H

#include "sgpr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGPR_LANDMARK_MAX_LABELS 64

size_t sgpr_landmark_workspace_bytes(int G, int N);

int sgpr_landmark_map(const float* d_centers, const int32_t* d_labels, int G, int N, const double* d_poses,
                      const int32_t* h_starts, int n_sessions, const double* h_radius, int n_labels, double tau_z,
                      int max_landmarks, double* d_lm_center, int32_t* d_lm_label, int32_t* d_lm_count,
                      int32_t* d_lm_first, uint64_t* d_lm_sessions, double* d_lm_spread, int32_t* d_node_landmark,
                      int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARKS_H */
