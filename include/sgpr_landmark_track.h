/*
 * sgpr_landmark_track.h - track drives through a landmark map: odometry predicts every scan's pose, the map corrects it,
 * scan by scan (libsgpr_hip.so).  A ninth public header in the style of sgpr_landmark_align.h: the
 * conventions and error codes of sgpr.h hold here, and neither sgpr.h (its 100 functions, SGPR_ABI_VERSION) nor any of
 * the seven other headers (sgpr_posegraph.h, sgpr_localize.h, sgpr_landmarks.h, sgpr_landmark_refine.h,
 * sgpr_landmark_align.h, sgpr_landmark_update.h, sgpr_landmark_persist.h) is changed by it.
 *
 * sgpr_landmark_track takes the packed node arrays of Q scans of N slots, the odometry pose of every scan in a frame of
 * its drive's own, a host table that cuts the Q scans into tracks, the map-frame pose of every track's FIRST scan, and the
 * landmarks of a map exactly as sgpr_landmark_align takes them.  The scans of a track are aligned in order: scan i starts
 * from the aligned pose of scan i - 1 moved by the odometry between the two, runs a schedule of gates - each stage one
 * sgpr_landmark_align of that scan - and is accepted, or LOST: then it falls back to its prediction and the next scan
 * runs wider re-acquisition gates first.  Tracks are independent of one another; the scans of a track are not.
 *
 * ARITHMETIC.  Float64, every operation rounded on its own: no fused multiply-add, division and sqrt correctly rounded.
 * The result is reproducible bit for bit (tests/landmark_track_ref.py is this text in NumPy).
 *
 * TRACKS.  h_starts [n_tracks] as the session table of sgpr_landmark_map: h_starts[0] == 0, non-decreasing, every entry
 * at most Q, n_tracks in 1..SGPR_SESSION_MAX; track t is the scans [h_starts[t], h_starts[t + 1]), the last one runs to Q;
 * a repeated entry is an empty track.  NULL with n_tracks == 0: one track of all Q scans.  d_init holds one pose per track
 * (one pose when there is no table).
 *
 * POSES are planar (c, s, x, y).  With a = (ac, as, ax, ay) and b likewise,
 *   a o b  = (ac bc - as bs,  as bc + ac bs,  (ac bx - as by) + ax,  (as bx + ac by) + ay)
 *   inv(a) = (ac,  -as,  -(ac ax + as ay),  as ax - ac ay)
 * every product, sum and difference rounded once, in the order written; nothing is renormalised.
 *
 * Scan i of track t, in ascending i; A_i is its output pose, P_i its prediction, O_i = d_odom[i]:
 *
 * 1. PREDICTION.  i is the first scan of the track: P_i = d_init[t].  Otherwise
 *      P_i = A_{i-1} o (inv(O_{i-1}) o O_i),
 *    unless any of the eight doubles of O_{i-1} and O_i is not finite: then P_i = A_{i-1} bit for bit and flags bit 3
 *    (NO_ODOM, value 8) is set.
 *
 * 2. STAGES.  X = P_i.  Stage j, j = 0 .. n_stages - 1, has the radii h_radius[j n_labels .. (j + 1) n_labels).  Stages
 *    n_reacquire .. n_stages - 1 run on every scan, in ascending j.  Stages 0 .. n_reacquire - 1 run in front of them, but
 *    only when n_reacquire > 0 and the previous scan of the track was LOST - for the first scan of a track: when `flags`
 *    has SGPR_TRACK_START_LOST - and then flags bit 4 (REACQUIRE, value 16) is set.  A stage is, to the letter,
 *    sgpr_landmark_align of this one scan (Q = 1) from d_poses = X with that stage's radii and the call's tau_z, iters
 *    and min_nodes: its map point, live and eligible rules (eligible under THAT stage's radii), the match by (d2, id),
 *    the sum W, the fit, the keep rule and the rule for a non-finite X.  X becomes that call's d_poses_out.
 *
 * 3. ACCEPT OR REJECT.  matched, live, d_rms[i] and the row d_node_landmark[i N ..] are those of the last stage (counted
 *    under the final X); refits is the sum of the refits of the stages run; flags bit 1 (KEPT, 2) and bit 0 (NONFINITE, 1)
 *    are the OR over the stages run.  With dx = X.x - P_i.x, dy = X.y - P_i.y, the scan is LOST - flags bit 2, value 4 -
 *    when
 *      matched < min_matched   or   dx dx + dy dy > max_shift max_shift,
 *    the right-hand product formed once (max_shift = +inf: never; a NaN on the left: not lost by this test).
 *    LOST: A_i = P_i bit for bit.  Otherwise A_i = X.
 *
 * 4. NON-FINITE d_init[t] (any of its four doubles).  Every scan i of the track: d_poses_out[i] = d_pred_out[i] =
 *    d_init[t] bit for bit, every node -1, d_stat[i] = (0, 0, 0, 1) - NONFINITE alone - and d_rms[i] the quiet NaN
 *    0x7ff8000000000000.  Such a scan is neither tracked nor lost.
 *
 * OUTPUTS.  d_poses_out [Q,4] = A.  d_pred_out [Q,4] = P.  d_node_landmark [Q,N].  d_stat [Q,4] = (matched, live, refits,
 * flags).  d_rms [Q].  d_num [4] = (scans tracked: flags has neither LOST nor NONFINITE; scans lost; the longest run of
 * consecutive LOST scans inside one track; tracks that are not empty).
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation; the radii and the table are HOST arrays and are copied into the launch.  The results depend on the
 * arguments alone, on any stream: the workspace need not be initialised.  It needs
 * sgpr_landmark_track_workspace_bytes(Q, N, L, n_stages) bytes, 256-byte aligned: n_stages times
 * sgpr_landmark_align_workspace_bytes(Q, N, L) - every stage has a search table of its own, with cells as wide as ITS
 * radii ask for: lm_cell_width(r) = max(1.001 r, 0.5) per label, as in sgpr_landmark_align - and 0 when Q N is 0 or an
 * argument is out of range.  No output may overlap an input or another output.
 * Checked before the device is touched, SGPR_E_INVALID with a message naming the fault: Q, N, L or iters < 0;
 * n_stages outside 1..SGPR_TRACK_MAX_STAGES; n_reacquire outside 0..n_stages - 1; min_nodes < 2; min_matched < 0;
 * n_labels outside 1..SGPR_LANDMARK_MAX_LABELS; a NULL h_radius; a negative or NaN radius (+inf is a radius); a negative
 * or NaN tau_z or max_shift (+inf disables the shift test); a bad track table (the rules above); Q N > 2^31 - 1; with
 * Q N > 0, a NULL device pointer (d_lm_use may be NULL: every landmark takes part; d_lm_center and d_lm_label may be NULL
 * when L is 0) or a workspace that is too small.  Q == 0 or N == 0 succeeds without touching the device: NOTHING is
 * written then.
 */
#ifndef SGPR_LANDMARK_TRACK_H
#define SGPR_LANDMARK_TRACK_H

#include "sgpr.h"
#include "sgpr_landmarks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGPR_TRACK_MAX_STAGES 4

/* `flags` of the call */
#define SGPR_TRACK_START_LOST 1

/* flags of a scan (d_stat[i][3]) */
#define SGPR_TRACK_NONFINITE 1
#define SGPR_TRACK_KEPT 2
#define SGPR_TRACK_LOST 4
#define SGPR_TRACK_NO_ODOM 8
#define SGPR_TRACK_REACQUIRE 16

size_t sgpr_landmark_track_workspace_bytes(int Q, int N, int L, int n_stages);

int sgpr_landmark_track(const float* d_centers, const int32_t* d_labels, int Q, int N, const double* d_odom,
                        const int32_t* h_starts, int n_tracks, const double* d_init, const double* d_lm_center,
                        const int32_t* d_lm_label, const uint8_t* d_lm_use, int L, const double* h_radius, int n_stages,
                        int n_reacquire, int n_labels, double tau_z, int iters, int min_nodes, int min_matched,
                        double max_shift, int flags, double* d_poses_out, double* d_pred_out, int32_t* d_node_landmark,
                        int32_t* d_stat, double* d_rms, int32_t* d_num, void* d_workspace, size_t workspace_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LANDMARK_TRACK_H */
