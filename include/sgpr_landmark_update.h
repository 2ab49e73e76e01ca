/*
 * sgpr_landmark_update.h - fold further scans into a landmark map: an incremental update of the records
 * (libsgpr_hip.so).  A seventh public header in the style of sgpr_landmark_align.h: the conventions, error
 * codes and SESSION TABLE rules of sgpr.h hold here, and neither sgpr.h (its 100 functions, SGPR_ABI_VERSION) nor
 * sgpr_posegraph.h (its two functions) nor sgpr_localize.h (its one) nor sgpr_landmarks.h (its two) nor
 * sgpr_landmark_refine.h (its two) nor sgpr_landmark_align.h (its two) is changed by it.
 *
 * sgpr_landmark_update takes the packed node arrays of Q scans of N slots, one planar pose per scan in the frame of the
 * map (the poses sgpr_landmark_align left), the association of every node with the map (what sgpr_landmark_align wrote to
 * d_node_landmark: a landmark id, -2 for a live node the map does not explain, -1 for a dead one) and the L records of the
 * map (the outputs of sgpr_landmark_map, or of an earlier update).  A node associated with a landmark becomes one more
 * observation of it: count, centre, sessions and spread of the record move as if the node had been a member.  The nodes
 * the map does not explain are fused among themselves into NEW landmarks L, L+1, .. exactly as sgpr_landmark_map fuses
 * the nodes of a map.  Old landmarks keep their ids, never merge and are never removed, so every node_landmark array,
 * mask and virtual scan made on the map before stays valid.
 *
 * ARITHMETIC.  Float64, every operation rounded on its own: no fused multiply-add, division and sqrt correctly rounded.
 * Every sum over nodes is an INTEGER sum of fixed-point values, so nothing depends on the order of execution.  The result
 * is reproducible bit for bit (tests/landmark_update_ref.py is this text in NumPy).
 *
 * MAP POINT of node (q, n), flat index p = q N + n, and LIVE node: exactly those of sgpr_landmarks.h under d_poses[q],
 * with its radius-table rule (0 <= label < n_labels and h_radius[label] > 0) and its limit of 2^37 m.
 *
 * ELIGIBLE landmark id, with (center, label, count, spread) its record: 0 <= label < n_labels and h_radius[label] > 0;
 * 1 <= count <= 262144 (2^18); the three centre doubles are finite; with n0 = double(count), |center_k n0| <= 2^38 for
 * every k (so that the recovered sum below fits 64 bits); spread is finite and >= 0 (-0.0 is).
 *
 * OBSERVATION: a live node whose d_assoc names an id in [0, L) that is eligible and carries the node's label.
 * NEW NODE: a live node with d_assoc == -2.
 * REJECTED NODE: every other live node - any other value, an ineligible landmark, another label.  It gets -1, as a dead
 * node does, and changes nothing.
 *
 * RECORD of an old landmark with n1 >= 1 observations O, m the map point of an observation:
 *   S_k       = llrint((center_k n0) 2^24) + the sum over O of llrint(m_k 2^24), an int64 sum that wraps
 *   count'    = count + n1
 *   center'_k = double(S_k) / (double(count') * 16777216.0)
 *   sessions' = sessions | the OR over O of (1 << (session_base + session(q))),  session(q) = the largest j with
 *               h_starts[j] <= q (0 without a table): the session rule of sgpr.h over the Q scans
 *   label, first   copied
 *   spread'   = sqrt(double(Q') / (double(count') * 16777216.0))
 *   Q'        = (uint64) llrint((min(v, 2^20) n0) 2^24) + the sum over O of llrint(min(d2, 2^20) 2^24), a uint64 sum
 *   v         = spread spread + (ax ax + ay ay),  a = center - center' in x and y: the parallel-axis theorem, the mean
 *               squared planar distance of the old members about the NEW centre without their coordinates
 *   d2        = ex ex + ey ey,  ex = mx - center'_0, ey = my - center'_1
 * An old landmark without an observation, and an ineligible one, is copied bit for bit.
 *
 * NEW LANDMARKS.  The new nodes are linked among themselves by the LINK rule of sgpr_landmarks.h (same label, h_radius,
 * tau_z).  The connected components are numbered L, L+1, .. by ascending lowest flat node index p.  Each gets the RECORD
 * of sgpr_landmarks.h over its members with two changes: first = node_base + p, and the session bits are shifted by
 * session_base.  A new node never joins an old landmark here, whatever its distance to one.
 *
 * OUTPUTS.  d_node_landmark[p] = the id in the updated map: the old id of an observation, the new id of a new node, -1
 * otherwise.  d_num = (L', live nodes, observations, new nodes), L' = L + the number of new landmarks.  L' may exceed
 * max_landmarks: then only the records below max_landmarks are written - every byte of those, nothing past them - and the
 * node ids are complete all the same.  Each d_out_* array may be the corresponding d_lm_* array (an update in place);
 * otherwise it may not overlap any input.  d_node_landmark may be d_assoc.
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation; the session table and the radii are HOST arrays and are copied into the launches.  The results depend
 * on the arguments alone, on any stream: the workspace need not be initialised.  It needs
 * sgpr_landmark_update_workspace_bytes(Q, N, L) bytes, 256-byte aligned (0 when Q N is 0 or an argument is out of range).
 * Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: Q, N, L, max_landmarks, node_base
 * or session_base < 0; max_landmarks < L; session_base + max(n_sessions, 1) > 64; node_base + Q N > 2^31 - 1, or
 * Q N > 2^30 (so that count' fits int32); n_labels outside 1..SGPR_LANDMARK_MAX_LABELS; a NULL h_radius; a negative or NaN
 * radius (+inf is a radius); a negative or NaN tau_z; a bad session table (of the Q scans); with Q N > 0, a NULL device
 * pointer (the six d_out_* arrays may be NULL when max_landmarks is 0, the six d_lm_* arrays when L is 0) or a workspace
 * that is too small.  Q == 0 or N == 0 succeeds without touching the device: NOTHING is written then, d_num included -
 * the map is what it was.
 */
#ifndef SGPR_LANDMARK_UPDATE_H
#define SGPR_LANDMARK_UPDATE_H

#include "sgpr.h"
#include "sgpr_landmarks.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t sgpr_landmark_update_workspace_bytes(int Q, int N, int L);

int sgpr_landmark_update(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_poses,
                         const int32_t* d_assoc, const int32_t* h_starts, int n_sessions, int session_base, int node_base,
                         const double* h_radius, int n_labels, double tau_z, const double* d_lm_center,
                         const int32_t* d_lm_label, const int32_t* d_lm_count, const int32_t* d_lm_first,
                         const uint64_t* d_lm_sessions, const double* d_lm_spread, int L, int max_landmarks,
                         double* d_out_center, int32_t* d_out_label, int32_t* d_out_count, int32_t* d_out_first,
                         uint64_t* d_out_sessions, double* d_out_spread, int32_t* d_node_landmark, int32_t* d_num,
                         void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARK_UPDATE_H */
