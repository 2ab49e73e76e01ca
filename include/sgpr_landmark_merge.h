/*
 * sgpr_landmark_merge.h - join and compact landmark maps: a merge of the records alone (libsgpr_hip.so).
 * An eleventh public header in the style of sgpr_landmark_update.h: the conventions and error codes of sgpr.h hold here,
 * and neither sgpr.h (its 100 functions, SGPR_ABI_VERSION) nor any of the ten headers before this one is changed by it.
 *
 * sgpr_landmark_merge takes the records of a map A (L_a landmarks: the outputs of sgpr_landmark_map, of
 * sgpr_landmark_update or of an earlier merge), optionally the records of a second map B (L_b landmarks) with the planar
 * pose that carries B's frame into A's, and a keep mask per map (what sgpr_landmark_persist wrote, or any other).  It
 * drops what a mask drops, fuses the records of one label that lie within that label's radius as if their observations
 * had been fused, numbers the result densely and says where every old id went.  No node arrays are read.  With L_b = 0
 * the call compacts A; with two maps it joins them.
 *
 * ARITHMETIC.  Float64, every operation rounded on its own: no fused multiply-add, division and sqrt correctly rounded.
 * Every sum over records is an INTEGER sum of fixed-point values, so nothing depends on the order of execution.  The
 * result is reproducible bit for bit (tests/landmark_merge_ref.py is this text in NumPy).
 *
 * The inputs are indexed i in [0, L_a) for A's records and L_a + j for record j of B.
 *
 * INPUT RECORD.  A's record is taken as it is.  B's record has its centre (x, y, z) moved by h_pose = (c, s, X, Y):
 *   px = (c x - s y) + X,  py = (s x + c y) + Y,  pz = z;
 * its sessions become sessions << session_shift (bits shifted out are lost) and its first becomes first + first_base
 * (int32, wrapping).  With h_pose == NULL B's centres are taken bit for bit; that is not the identity pose, which turns
 * -0.0 into +0.0.
 *
 * KEPT: the keep pointer of the record's map is NULL, or keep[i] != 0.
 * ELIGIBLE: kept, and on the input record (centre p, label, count, spread): 0 <= label < n_labels and
 *   h_radius[label] > 0; 1 <= count <= 262144 (2^18); the three centre doubles are finite and, with n = double(count),
 *   |p_k n| <= 2^38 for every k; spread is finite and >= 0 (-0.0 is).  Every record that is not eligible is DROPPED.
 *
 * LINK.  Eligible records i != j of one label l link iff dx dx + dy dy <= r r (dx = px_i - px_j, dy likewise, r =
 * h_radius[l], the product r r formed once) and |pz_i - pz_j| <= tau_z.  The test is symmetric in its bits, and it
 * applies inside A, inside B and across the two.
 *
 * OUTPUT LANDMARK: a connected component of the link graph.  The components are numbered 0 .. L' - 1 by ascending
 * lowest input index: a map that loses no record and fuses none keeps its ids, a map that only loses records keeps
 * their order.  d_old_to_new[L_a + L_b] = the new id of every input record, -1 of a dropped one.
 *
 * RECORD of a component of ONE member: the input record, bit for bit.
 * RECORD of a component of several members i, with n_i = double(count_i):
 *   sum       = the int64 sum of the counts;  count' = min(sum, 2^31 - 1);  every division below uses double(sum)
 *   S_k       = the int64 sum, which wraps, of llrint((p_ik n_i) 2^24)
 *   center'_k = double(S_k) / (double(sum) * 16777216.0)
 *   sessions' = the OR of the members' sessions;  first' = the lowest first;  label copied
 *   Q'        = the uint64 sum of (uint64) llrint((min(v_i, 2^20) n_i) 2^24),  v_i = spread_i spread_i + (ax ax + ay ay),
 *               a = p_i - center' in x and y: the parallel-axis theorem, the mean squared planar distance of a member's
 *               observations about the NEW centre without their coordinates
 *   spread'   = sqrt(double(Q') / (double(sum) * 16777216.0))
 *
 * OUTPUTS.  d_num = (L', records dropped by a keep mask, kept records dropped as ineligible, components of more than one
 * member).  L' may exceed max_out: then only the records below max_out are written - every byte of those, nothing past
 * them - and d_old_to_new and d_num are complete all the same.  No output may overlap an input: the renumbering rules
 * out a call in place.
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation; the pose and the radii are HOST arrays and are copied into the launches.  The results depend on the
 * arguments alone, on any stream: the workspace need not be initialised.  It needs
 * sgpr_landmark_merge_workspace_bytes(L_a, L_b) bytes, 256-byte aligned (0 when L_a + L_b is 0 or an argument is out of
 * range).  Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: L_a, L_b, max_out or
 * first_base < 0; L_a + L_b > 2^31 - 1; session_shift outside 0..63; n_labels outside 1..SGPR_LANDMARK_MAX_LABELS; a NULL
 * h_radius; a negative or NaN radius (+inf is a radius); a negative or NaN tau_z; an h_pose with a value that is not
 * finite; with L_a + L_b > 0, a NULL device pointer (the six records of a map may be NULL when it has no landmark, the
 * six d_out_* arrays when max_out is 0; a keep mask is always optional) or a workspace that is too small.
 * L_a + L_b == 0 succeeds without touching the device: NOTHING is written then, d_num included.
 */
#ifndef SGPR_LANDMARK_MERGE_H
#define SGPR_LANDMARK_MERGE_H

#include "sgpr.h"
#include "sgpr_landmarks.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t sgpr_landmark_merge_workspace_bytes(int L_a, int L_b);

int sgpr_landmark_merge(const double* d_a_center, const int32_t* d_a_label, const int32_t* d_a_count,
                        const int32_t* d_a_first, const uint64_t* d_a_sessions, const double* d_a_spread,
                        const uint8_t* d_keep_a, int L_a, const double* d_b_center, const int32_t* d_b_label,
                        const int32_t* d_b_count, const int32_t* d_b_first, const uint64_t* d_b_sessions,
                        const double* d_b_spread, const uint8_t* d_keep_b, int L_b, const double* h_pose,
                        int session_shift, int first_base, const double* h_radius, int n_labels, double tau_z,
                        int max_out, double* d_out_center, int32_t* d_out_label, int32_t* d_out_count,
                        int32_t* d_out_first, uint64_t* d_out_sessions, double* d_out_spread, int32_t* d_old_to_new,
                        int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARK_MERGE_H */
