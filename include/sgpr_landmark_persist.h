/*
 * sgpr_landmark_persist.h - which landmarks of a map did a drive see, and which should it have seen: visibility tallies
 * and a retire mask (libsgpr_hip.so).  An eighth public header in the style of sgpr_landmark_align.h and
 * sgpr_landmark_update.h: the conventions and error codes of sgpr.h hold here, and neither sgpr.h (its 100 functions,
 * SGPR_ABI_VERSION) nor sgpr_posegraph.h (its two functions) nor sgpr_localize.h (its one) nor sgpr_landmarks.h (its two)
 * nor sgpr_landmark_refine.h (its two) nor sgpr_landmark_align.h (its two) nor sgpr_landmark_update.h (its two) is changed
 * by it.
 *
 * sgpr_landmark_persist takes the packed node arrays of Q scans of N slots, one planar pose per scan in the frame of the
 * map (the poses sgpr_landmark_align left), the association of every node with the map (d_node_landmark of
 * sgpr_landmark_align or of sgpr_landmark_update) and the landmarks of the map (centre, label and a mask of those that
 * take part).  A scan sees what lies within the range of its farthest node, capped by the sensor range; for every
 * landmark the call counts the scans that SHOULD have seen it and the scans that DID, and marks the landmarks the drive
 * should have seen and did not.  The mark is a mask: no record is removed, renumbered or changed.  There is no occlusion
 * model - a landmark hidden behind a lorry counts as missed; the margin and the ratio absorb that.
 *
 * ARITHMETIC.  Float64, every operation rounded on its own: no fused multiply-add, sqrt correctly rounded.  Every tally
 * is an INTEGER count and the view range a maximum, so nothing depends on the order of execution.  The result is
 * reproducible bit for bit (tests/landmark_persist_ref.py is this text in NumPy).
 *
 * MAP POINT of node (q, n) and LIVE node: exactly those of sgpr_landmark_align.h at k = 0 under X = d_poses[q] =
 * (c, s, X, Y).  A scan with a non-finite pose has no live node.
 *
 * ELIGIBLE landmark: exactly that of sgpr_landmark_align.h - d_lm_use is NULL or d_lm_use[id] != 0; 0 <= d_lm_label[id]
 * < n_labels and h_radius of that label > 0; its three centre doubles are finite and at most 2^37 in magnitude.
 *
 * VIEW RANGE of scan q:  far2_q = the maximum over the live nodes of the scan of x x + y y, (x, y) the node's centre
 * widened from float32 - the SENSOR frame: it does not depend on the pose - and 0.0 without a live node;
 *   v_q = min(max_range, sqrt(far2_q)) - margin,     d_view[q] = v_q.
 *
 * IN VIEW(q, l), l eligible with centre (cx, cy, .):  v_q > 0  and  dx dx + dy dy <= v_q v_q,  dx = cx - X, dy = cy - Y,
 * the right-hand product formed once per scan.
 *
 * OBSERVED(q, l): some live node of scan q has d_assoc == l, 0 <= l < L, l eligible and of the node's label - the
 * OBSERVATION rule of sgpr_landmark_update.h without its count and spread conditions.  Several nodes of one scan on one
 * landmark are ONE observation: scans are counted, not nodes.  Every other association value is ignored.
 *
 * TALLIES.  d_expected[l] = the number of scans q with IN VIEW(q, l) or OBSERVED(q, l); d_seen[l] = the number with
 * OBSERVED(q, l); so seen <= expected.  An ineligible landmark gets 0 and 0.
 *
 * DECISION.  d_keep[l] = 0 - the landmark is RETIRED - when l is eligible, expected >= min_expected and
 * double(seen) < max_seen_ratio * double(expected); 1 otherwise (equality keeps).  It is made on THIS call's tallies:
 * on the drive passed in.
 *
 * d_scan_stat[q] = (the eligible landmarks IN VIEW or OBSERVED, the eligible landmarks OBSERVED, the live nodes, flags:
 * bit 0 NONFINITE (value 1) when any of the four doubles of the pose is not finite).  The ratio of the first two says how
 * much of what the map promised the scan found.
 * d_num = (landmarks retired, eligible landmarks with expected >= min_expected, eligible landmarks, scans with v_q > 0).
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation; the radii are a HOST array and are copied into the launches.  The results depend on the arguments
 * alone, on any stream: the workspace need not be initialised.  It needs sgpr_landmark_persist_workspace_bytes(Q, N, L)
 * bytes, 256-byte aligned:
 *   3 a(4 L) + a(8 H) + 2 a(4 H) + 256,   a(v) = v rounded up to a multiple of 256,
 *   H = the smallest power of two that is at least 1024 and at least 2 L
 * (0 when Q N is 0 or an argument is out of range).  No output may overlap an input or another output.
 * Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: Q, N, L or min_expected < 0;
 * Q N > 2^31 - 1; n_labels outside 1..SGPR_LANDMARK_MAX_LABELS; a NULL h_radius; a negative or NaN radius (+inf is a
 * radius); max_range negative or NaN (+inf is a range); margin negative or not finite; max_seen_ratio NaN or outside
 * [0, 1]; with Q N > 0, a NULL device pointer (d_lm_use may be NULL: every landmark takes part; d_lm_center, d_lm_label,
 * d_expected, d_seen and d_keep may be NULL when L is 0) or a workspace that is too small.
 * Q == 0 or N == 0 succeeds without touching the device: NOTHING is written then.  L == 0 with scans present writes
 * d_scan_stat, d_view and d_num only.
 */
#ifndef SGPR_LANDMARK_PERSIST_H
#define SGPR_LANDMARK_PERSIST_H

#include "sgpr.h"
#include "sgpr_landmarks.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t sgpr_landmark_persist_workspace_bytes(int Q, int N, int L);

int sgpr_landmark_persist(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_poses,
                          const int32_t* d_assoc, const double* d_lm_center, const int32_t* d_lm_label,
                          const uint8_t* d_lm_use, int L, const double* h_radius, int n_labels,
                          double max_range, double margin, int min_expected, double max_seen_ratio,
                          int32_t* d_expected, int32_t* d_seen, uint8_t* d_keep, int32_t* d_scan_stat,
                          double* d_view, int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARK_PERSIST_H */
