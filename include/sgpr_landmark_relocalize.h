/*
 * sgpr_landmark_relocalize.h - relocalise scans in a landmark map with no prior pose: global registration by the
 * consensus of pair hypotheses, refined by the alignment of sgpr_landmark_align.h (libsgpr_hip.so).  A
 * tenth public header in the style of sgpr_landmark_align.h: the conventions and error codes of sgpr.h hold here, and
 * neither sgpr.h (its 100 functions, SGPR_ABI_VERSION) nor any of the eight other headers (sgpr_posegraph.h,
 * sgpr_localize.h, sgpr_landmarks.h, sgpr_landmark_refine.h, sgpr_landmark_align.h, sgpr_landmark_update.h,
 * sgpr_landmark_persist.h, sgpr_landmark_track.h) is changed by it.
 *
 * sgpr_landmark_relocalize takes the packed node arrays of Q query scans of N slots and the landmarks of a map exactly
 * as sgpr_landmark_align takes them - and NO pose.  Two nodes of a scan are laid on two landmarks of their labels whose
 * distance agrees with theirs; that fixes a planar pose, and the nodes of the scan that find a landmark under it are
 * counted.  The hypothesis with the largest count wins, the best count at ANOTHER place is reported beside it (a
 * repeated constellation shows there), and the winning pose is refined by a schedule of alignment gates.  Every scan is
 * independent of every other: no output of one scan depends on another, or on the order of the scans.
 *
 * ARITHMETIC.  Float64, every operation rounded on its own: no fused multiply-add, division and sqrt correctly rounded.
 * Centres are widened from float32.  The result is reproducible bit for bit (tests/landmark_relocalize_ref.py is this
 * text in NumPy).  MAP POINT, ELIGIBLE, MATCH, FIT and W below are those of sgpr_landmark_align.h.
 *
 * LIVE node (q, n), centre (x, y, z), label l: 0 <= l < n_labels and h_radius_in[l] > 0; x, y, z finite and at most 2^37
 * in magnitude.  (A planar pose leaves z alone: whether a node is live does not depend on the hypothesis.)
 *
 * ELIGIBLE landmark: the rule of sgpr_landmark_align.h under h_radius_in.
 *
 * BASE PAIR (i, i'): live slots i < i' of the scan.  u = p_i' - p_i in the plane, lu = sqrt(ux ux + uy uy).  ADMISSIBLE
 * when min_base <= lu and lu <= max_base.
 *
 * HYPOTHESIS (i, i', j, j') of an admissible base pair: eligible landmarks j != j' with label(j) == label(i) and
 * label(j') == label(i'), centres (cx, cy, cz) and (cx', cy', cz');
 *   |z_i - cz| <= tau_z  and  |z_i' - cz'| <= tau_z;
 *   v = c_j' - c_j in the plane, lv = sqrt(vx vx + vy vy),  |lu - lv| <= tau_edge;
 *   den = lu lv is finite and > 0;
 *   c = (ux vx + uy vy) / den,  s = (ux vy - uy vx) / den     (nothing is renormalised);
 *   pm = 0.5 (p_i + p_i'),  lm = 0.5 (c_j + c_j')  per planar component;
 *   X = lmx - (c pmx - s pmy),  Y = lmy - (s pmx + c pmy);
 *   c, s, X, Y are all finite.
 * (c, s, X, Y) is its COARSE POSE.  A quadruple that fails any line is no hypothesis: it is neither counted nor evaluated.
 *
 * INLIERS of a hypothesis: the live nodes whose map point (mx, my, mz) under the coarse pose has mx, my at most 2^37 in
 * magnitude and for which a MATCH exists with r = h_radius_in[label] and tau_z - `matched` of sgpr_landmark_align with
 * iters = 0, h_radius = h_radius_in and that pose.
 *
 * ENUMERATION AND CAP.  The admissible base pairs are taken in ascending (i, i').  Before one is started: when the
 * hypotheses evaluated so far number max_hyp or more, the enumeration stops there and flags bit 2 (TRUNCATED, value 4)
 * is set.  A base pair that is started is never cut short: every one of its hypotheses is evaluated.  d_hyp[q] (int64)
 * is the number of hypotheses evaluated, d_stat[q][6] the number of admissible base pairs started, saturating at 2^31 - 1
 * (N is not limited; a scan of more than 65 536 live nodes can start more pairs than an int32 counts).
 *
 * WINNER: the evaluated hypothesis that comes first by the key (inliers DESCENDING, then i, i', j, j' ASCENDING) - a
 * maximum over one total order, so no order of evaluation can matter.  d_win[q] = its (i, i', j, j') - slots of the
 * scan, ids of the map -, d_coarse[q] its coarse pose, d_stat[q][0] its inliers.  No hypothesis evaluated: d_win[q] is
 * four times -1, d_coarse[q] four quiet NaNs 0x7ff8000000000000, inliers 0, and flags bit 3 (NO_HYPOTHESIS, value 8).
 *
 * FOUND - flags bit 0, value 1 - when there is a winner and its inliers >= min_inliers.
 *
 * OTHER PLACE (FOUND only; otherwise d_stat[q][1] = 0 and d_other[q] is four quiet NaNs).  Among the evaluated
 * hypotheses whose coarse (X, Y) has  dx dx + dy dy > sep sep  against the winner's coarse (X, Y), dx = X - Xw,
 * dy = Y - Yw, the right-hand product formed once, the first by the same key: d_stat[q][1] = its inliers, d_other[q] its
 * coarse pose.  There may be none (sep = +inf: never one): 0 and four quiet NaNs.
 *
 * REFINEMENT (FOUND only).  X = the winner's coarse pose.  Stage k = 0 .. n_stages - 1 in turn is, to the letter,
 * sgpr_landmark_align of this one scan (Q = 1) from d_poses = X with h_radius = h_radii[k n_labels .. (k + 1) n_labels),
 * the call's tau_z, iters and min_nodes (eligible under THAT stage's radii); X becomes its d_poses_out.
 * d_poses_out[q] = X.  matched, live, d_rms[q] and the row d_node_landmark[q N ..] are those of the last stage; refits
 * is the sum over the stages; flags bit 1 (KEPT, value 2) is the OR over the stages.  n_stages == 0: X stays the coarse
 * pose, and matched, live, d_rms[q] and the row are those of sgpr_landmark_align with iters = 0 and h_radius_in from it
 * (matched == inliers then).
 *
 * NOT FOUND.  d_poses_out[q] is four quiet NaNs, the row is -2 for a live node and -1 for any other, d_rms[q] the quiet
 * NaN, matched and refits 0, live the number of live nodes.
 *
 * OUTPUTS.  d_poses_out, d_coarse, d_other [Q,4].  d_node_landmark [Q,N].  d_stat [Q,8] = (inliers, inliers of the other
 * place, matched, live, refits, flags, admissible base pairs started, 0).  d_win [Q,4].  d_hyp [Q] int64.  d_rms [Q].
 * d_num [4] = (scans FOUND, scans TRUNCATED, scans with NO_HYPOTHESIS, 0).
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation; the radii are HOST arrays and are copied into the launches.  The results depend on the arguments
 * alone, on any stream: the workspace need not be initialised.  It needs
 * sgpr_landmark_relocalize_workspace_bytes(Q, N, L, n_stages) bytes, 256-byte aligned: n_stages + 2 times
 * sgpr_landmark_align_workspace_bytes(Q, N, L) - a search table under h_radius_in, one per stage, and the table that
 * finds j' around j, its cells lm_cell_width(max_base + tau_edge) wide -, 512 bytes of label counts, 512 n_stages bytes
 * of stage radii and, when N > 256, 4 Q N bytes rounded up to 256 for the live slots of every scan; 0 when Q N is 0 or an
 * argument is out of range.  No output may overlap an input or another output.
 * Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: Q, N, L or iters < 0; n_stages
 * outside 0..SGPR_RELOC_MAX_STAGES; n_labels outside 1..SGPR_LANDMARK_MAX_LABELS; a NULL h_radius_in, or a NULL h_radii
 * with n_stages > 0; a negative or NaN radius (+inf is a radius); a negative or NaN tau_z, tau_edge or min_base;
 * max_base below min_base, NaN or not finite; max_hyp < 1; min_inliers < 2; min_nodes < 2; a negative or NaN sep (+inf
 * is one); Q N > 2^31 - 1; with Q N > 0, a NULL device pointer (d_lm_use may be NULL: every landmark takes part;
 * d_lm_center and d_lm_label may be NULL when L is 0) or a workspace that is too small.  Q == 0 or N == 0 succeeds
 * without touching the device: NOTHING is written then.  L == 0 is a map like any other: every scan gets NO_HYPOTHESIS.
 */
#ifndef SGPR_LANDMARK_RELOCALIZE_H
#define SGPR_LANDMARK_RELOCALIZE_H

#include "sgpr.h"
#include "sgpr_landmarks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGPR_RELOC_MAX_STAGES 16

/* flags of a scan (d_stat[q][5]) */
#define SGPR_RELOC_FOUND 1
#define SGPR_RELOC_KEPT 2
#define SGPR_RELOC_TRUNCATED 4
#define SGPR_RELOC_NO_HYPOTHESIS 8

size_t sgpr_landmark_relocalize_workspace_bytes(int Q, int N, int L, int n_stages);

int sgpr_landmark_relocalize(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_lm_center,
                             const int32_t* d_lm_label, const uint8_t* d_lm_use, int L, const double* h_radius_in,
                             const double* h_radii, int n_stages, int n_labels, double tau_z, double tau_edge,
                             double min_base, double max_base, int max_hyp, int min_inliers, double sep, int iters,
                             int min_nodes, double* d_poses_out, double* d_coarse, double* d_other,
                             int32_t* d_node_landmark, int32_t* d_stat, int32_t* d_win, int64_t* d_hyp, double* d_rms,
                             int32_t* d_num, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARK_RELOCALIZE_H */
