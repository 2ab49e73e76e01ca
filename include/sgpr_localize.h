/*
 * sgpr_localize.h - the query side of the loop-closure pipeline: where is this scan in the map?  Pose consensus over
 * verified candidates (libsgpr_hip.so).  A third public header in the style of sgpr_posegraph.h: the
 * conventions, error codes and SESSION TABLE rules of sgpr.h hold here, and neither sgpr.h (its 100 functions,
 * SGPR_ABI_VERSION) nor sgpr_posegraph.h (its two functions) is changed by it.
 *
 * sgpr_localize_scans takes the planar poses of the map scans, the candidate map scans of every query scan with the
 * transforms sgpr_verify_pairs measured, and the query drive's own odometry.  Every candidate of the last L scans of
 * the query's session is one hypothesis of the query's pose in the map; the hypotheses of earlier scans are carried
 * forward by the odometry.  The answer is the mean of the largest set of hypotheses that agree with one of them, with
 * the size of that set as its support.
 *
 * ARITHMETIC.  All arithmetic is float64 and every operation is rounded on its own: no fused multiply-add, division and
 * sqrt correctly rounded.  An SE(2) element is (c, s, x, y), acting as p -> R p + t with R = [[c, -s], [s, c]].
 *   A o B (B first) = ( A.c B.c - A.s B.s,  A.s B.c + A.c B.s,  (A.c B.x - A.s B.y) + A.x,  (A.s B.x + A.c B.y) + A.y )
 *   inverse(A)      = ( A.c,  -A.s,  -(A.c A.x + A.s A.y),  A.s A.x - A.c A.y )
 * The result is reproducible bit for bit (tests/localize_ref.py is this text in NumPy).
 *
 * INPUTS.  d_map [M,4]: planar poses of the map scans in the map frame (X_out of sgpr_posegraph_optimize, or the planar
 * ground truth).  d_cols int32 [Q,K]: the candidate map scans of query i; any value outside 0..M-1 is padding (the -1 of
 * a top-k list included).  d_T [Q,K,4]: the `refined` field of sgpr_verify_pairs, a point of query scan i into map scan
 * cols[i,k], so the query's pose in the map is map[col] o T.  d_accept u8 [Q,K]: non-zero = the candidate takes part
 * (NULL = all do).  d_odo [Q,4]: planar odometry of the consecutive query scans in any frame of its own; read only when
 * L > 1 and may be NULL when L == 1.  h_starts, n_sessions: a HOST session table of the Q queries (NULL with 0 = one
 * session).  L in 1..SGPR_LOCALIZE_MAX_LEN, K in 1..SGPR_LOCALIZE_MAX_K (so L K <= 1024).
 *
 * HYPOTHESES of query i.  For l = 0..L-1 with i - l >= lo(i), the first query of i's session, and k = 0..K-1: slot
 * h = l K + k, j = i - l, col = cols[j,k].
 *   l = 0:  P_h = map[col] o T[j,k]                                        (no odometry is touched)
 *   l > 0:  P_h = (map[col] o T[j,k]) o (inverse(odo[j]) o odo[i])
 * Slot h is LIVE iff 0 <= col < M, the candidate is accepted and all four doubles of P_h are finite (a non-finite
 * input anywhere reaches P_h: this is the one test).  Every other slot of the L K is dead.
 *
 * AGREEMENT.  Live a and b agree iff  P_a.c P_b.c + P_a.s P_b.s >= min_cos  and  dx dx + dy dy <= max_trans max_trans,
 * dx = P_a.x - P_b.x, dy = P_a.y - P_b.y; the right-hand product is formed once.  The test is symmetric in bits.
 * support(a) = 1 + the number of live b != a that agree with a.
 *
 * WINNER.  The live slot with the largest support, ties to the lowest h.  Its supporters are itself and the slots that
 * agree with it.
 *
 * FUSED POSE.  P2 = the smallest power of two >= L K; v[h] = the value at a supporter slot, +0 elsewhere up to P2;
 * S(v) = the halving tree v[i] + v[i + half], half = P2/2 .. 1; n = support as a double.
 *   rotation     g = (S(c), S(s)) / sqrt(S(c)^2 + S(s)^2); if that norm is 0 or not finite, g is the winner's (c, s) and
 *                SGPR_LOCALIZE_DEGENERATE is set
 *   translation  t = (S(x) / n, S(y) / n)
 *   spread       sqrt(S((x_h - t.x)^2 + (y_h - t.y)^2) / n), each square formed on its own, then the two added
 *
 * OUTPUTS (every byte written for Q > 0).  d_pose [Q,4] = (g, t).  d_stat int32 [Q,4] = (support, live slots, winner h,
 * flags).  d_spread [Q].  Without a live slot: pose and spread are NaN and stat = (0, 0, -1, SGPR_LOCALIZE_NO_HYPOTHESIS).
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and uses no workspace, no
 * host synchronisation and no global atomics; the session table is copied into the launch.  Results depend on the
 * arguments alone, on any stream.  Checked before the device is touched, SGPR_E_INVALID with a message naming the fault:
 * a NULL pointer with Q > 0 (d_accept may always be NULL, d_odo only when L == 1), Q or M < 0, K or L out of range, a
 * bad session table, a negative or NaN max_trans, a NaN min_cos.  Q == 0 succeeds without a launch.  M == 0 with Q > 0
 * is valid: every slot is then padding.
 */
#ifndef SGPR_LOCALIZE_H
#define SGPR_LOCALIZE_H

#include "sgpr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGPR_LOCALIZE_MAX_K 64
#define SGPR_LOCALIZE_MAX_LEN 16

/* flags (stat[3]) */
#define SGPR_LOCALIZE_NO_HYPOTHESIS 1
#define SGPR_LOCALIZE_DEGENERATE 2

int sgpr_localize_scans(const double* d_map, int M, const int32_t* d_cols, const double* d_T, const uint8_t* d_accept,
                        int Q, int K, const double* d_odo, const int32_t* h_starts, int n_sessions, int L,
                        double max_trans, double min_cos, double* d_pose, int32_t* d_stat, double* d_spread,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_LOCALIZE_H */
