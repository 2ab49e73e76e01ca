/*
 * sgpr_posegraph.h - the back end of the loop-closure pipeline: planar pose-graph relaxation over accepted closures
 * (libsgpr_hip.so).  A second public header in the style of sgpr.h: its conventions, error codes
 * and SESSION TABLE rules hold here, and sgpr.h (its 100 functions, SGPR_ABI_VERSION) is not changed by it.
 *
 * sgpr_posegraph_optimize takes the stacked planar odometry of a (multi-session) map and the closure edges that
 * sgpr_verify_pairs measured and sgpr_consistent_set accepted, and returns one map in one frame with the drift spread
 * over the loops: a two-stage linear ("chordal") solve - rotations first, then translations - each stage a
 * preconditioned conjugate-gradient solve on a (connection) Laplacian over complex numbers.
 *
 * ARITHMETIC.  All arithmetic is float64 and every operation is rounded on its own: no fused multiply-add, division and
 * sqrt correctly rounded.  A complex product (a+ib)(c+id) is (ac - bd) + i(ad + bc); conj(z) v is
 * (z_r v_r + z_i v_i) + i(z_r v_i - z_i v_r); complex / real and real * complex act on each part.  The result is
 * reproducible bit for bit (tests/posegraph_ref.py is this text in NumPy).
 *
 * INPUTS.  d_X [M,4]: planar poses (c, s, x, y) of the stacked map, each scan into its session's own frame;
 * g0 = c + i s, t0 = x + i y.  h_starts, n_sessions: a HOST session table of the M scans (NULL with 0 = one session).
 * Closures p = 0..C-1: d_rows[p], d_cols[p] (int32 indices into X) and d_T [C,4] = (c, s, x, y), a point of scan rows[p]
 * into scan cols[p], i.e. X_rows = X_cols o T.  d_weight [C]: an optional multiplier (NULL = 1).  d_fixed u8 [M]:
 * non-zero = the scan keeps its pose (NULL = scan 0 alone).  Four weights w_odo_rot, w_odo_trans, w_clo_rot,
 * w_clo_trans; max_iters; rel_tol.
 *
 * EDGES i -> j with (zr, zt, w_rot, w_trans).
 *   odometry, for every k, k+1 of one session: q = conj(g0_k) g0_{k+1}, zr = q / sqrt(q_r^2 + q_i^2),
 *     zt = conj(g0_k)(t0_{k+1} - t0_k), weights w_odo_*;
 *   closure p: i = cols[p], j = rows[p], zr = (T.c + i T.s) / sqrt(T.c^2 + T.s^2), zt = T.x + i T.y, weights
 *     w_clo_* * weight[p].
 * A closure is LIVE iff both indices lie in 0..M-1, rows != cols, its four doubles are finite, T.c^2 + T.s^2 > 0 and its
 * multiplier is finite and > 0.  Any other closure is void and takes no part.
 *
 * STATUS (info[0]).  A non-finite double in X, or a scan with c^2 + s^2 == 0, sets SGPR_POSEGRAPH_NONFINITE; no fixed
 * scan sets SGPR_POSEGRAPH_NO_ANCHOR.  With either flag X_out is X bit for bit and every other word of info and resid
 * is 0.
 *
 * WHICH SCANS MOVE.  Two sessions are adjacent when a live closure joins them; a session is ACTIVE when it is reachable
 * from a session that holds a fixed scan; a scan is FREE when its session is active and it is not fixed.  Every other
 * scan keeps its input bits and enters the sums as a boundary value.  Without a live closure (C == 0 included) X_out
 * is X bit for bit, both stages are skipped (0 iterations, reason 0, resid 0) and info[5..7] are reported.
 *
 * THE OPERATOR OF A STAGE (unknown u, per-edge z, w, right-hand side rhs_e).  d_e(u) = w (u_j - z u_i); an edge
 * contributes +d_e at its head j and -conj(z) d_e at its tail i.  (A u)_k, b_k (from d_e = w rhs_e) and diag_k (the sum
 * of the w) are accumulated for a free k in this order, starting FROM the first term (not from 0):
 *   1. the odometry edge into k;  2. live closures with rows[p] = k, ascending p;
 *   3. the odometry edge out of k;  4. live closures with cols[p] = k, ascending p.
 * Non-free entries of A u, b, diag, and of the vectors r, p, zv of the iteration, are +0 and never updated; non-free
 * entries of u keep u0.
 *
 * THE PRECONDITIONER.  position(k) = k - starts[sess(k)].  The coupling lower_k = -(w z) of the odometry edge k-1 -> k
 * is kept iff both scans are free and position(k) % SGPR_POSEGRAPH_SEGMENT != 0.  Factor, ascending k: without a
 * coupling piv_k = diag_k; otherwise l_k = lower_k / piv_{k-1} and piv_k = diag_k - (l_r lower_r + l_i lower_i).
 * Apply: y = r; ascending k with a coupling: y_k -= l_k y_{k-1}; then y_k /= piv_k for every k; descending k where k+1
 * has a coupling: y_k -= conj(l_{k+1}) y_{k+1}; non-free entries -> +0.  Steps without a coupling are skipped, not
 * multiplied by zero.  Segments are independent.
 *
 * THE SUM S(v) over the M entries in scan order: consecutive chunks of 1024 entries, zero-padded, are each reduced by
 * the halving tree v[i] + v[i+h], h = 512 .. 1; the chunk sums, zero-padded to a power of two P, are reduced by the
 * same tree, h = P/2 .. 1.  <a, b> = S(a_r b_r + a_i b_i).
 *
 * THE ITERATION.  u = u0, r = b - A u, zv = M^-1 r, p = zv, rz0 = rz = <r, zv>, it = 0.  While it < max_iters and
 * rz > (rel_tol * rel_tol) * rz0 and rz > 0:  Ap = A p, pAp = <p, Ap>; stop with reason BREAKDOWN unless pAp > 0;
 * alpha = rz / pAp, u += alpha p, r -= alpha Ap; zv = M^-1 r, rzn = <r, zv>, p = zv + (rzn / rz) p, rz = rzn, it += 1.
 * Otherwise the reason is MAX_ITERS when the loop ended on it == max_iters with the other two conditions still true,
 * and CONVERGED when not.
 *
 * STAGE R.  u0 = g0, z = zr, the rotation weights, rhs = 0 (b = +0).  Afterwards a free g_k is divided by
 * n = sqrt(g_r^2 + g_i^2); if n is 0 or not finite, g_k = g0_k and SGPR_POSEGRAPH_DEGENERATE is set.
 * STAGE T.  u0 = t0, z = 1 (its products are skipped: d_e = w (u_j - u_i), the tail gets -d_e, lower_k = -w + 0i), the
 * translation weights, rhs_e = g_i zt_e with stage R's normalised g, and g0 at non-free scans.
 *
 * OUTPUTS.  d_X_out [M,4] (must not overlap d_X): (g, t) of a free scan, the input bits of every other.
 * d_info int32 [8]: 0 status flags; 1, 2 iterations of R, T; 3, 4 stop reason of R, T; 5 live closures; 6 free scans;
 * 7 active sessions.  d_resid double [4]: rz0, rz of R; rz0, rz of T.
 *
 * LIMITS.  M <= SGPR_POSEGRAPH_MAX_SCANS, C <= SGPR_POSEGRAPH_MAX_CLOSURES, max_iters in 0..SGPR_POSEGRAPH_MAX_ITERS.
 *
 * WORKSPACE.  sgpr_posegraph_optimize_workspace_bytes(M, C) =
 *     8192 + 192 M + 64 C + 2624 (M / 64 + 64)      (integer division; 0 for M == 0 or a count out of range)
 * bytes of device memory, aligned to 16 bytes: the vectors of the iteration, the edge quantities, the closure lists of
 * every scan and the position-major ([position][segment]) factor, of which a map has at most M / 64 + 64 segments.
 *
 * THE CALL is handle-free, runs on the caller's current device, is asynchronous on `stream` and makes no host
 * synchronisation: one persistent workgroup loops on the device and leaves when converged; the iteration counts are
 * read from d_info afterwards.  Checked before the device is touched, SGPR_E_INVALID with a message naming the fault
 * (and the workspace query answers 0): a NULL pointer with a positive count (d_info and d_resid always), M, C or
 * max_iters out of range, a bad session table, a weight that is not finite and positive, a negative or NaN rel_tol.
 * A missing or short workspace: SGPR_E_WORKSPACE.  M == 0 succeeds without a launch and writes nothing.  Otherwise every
 * byte of X_out, info and resid is written, and results depend on the arguments alone: any workspace contents, any
 * stream.
 */
#ifndef SGPR_POSEGRAPH_H
#define SGPR_POSEGRAPH_H

#include "sgpr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGPR_POSEGRAPH_MAX_SCANS 65536
#define SGPR_POSEGRAPH_MAX_CLOSURES 16384
#define SGPR_POSEGRAPH_MAX_ITERS 65536
#define SGPR_POSEGRAPH_SEGMENT 64

/* status flags (info[0]) */
#define SGPR_POSEGRAPH_NONFINITE 1
#define SGPR_POSEGRAPH_NO_ANCHOR 2
#define SGPR_POSEGRAPH_DEGENERATE 4

/* stop reasons (info[3], info[4]) */
#define SGPR_POSEGRAPH_CONVERGED 0
#define SGPR_POSEGRAPH_STOP_MAX_ITERS 1
#define SGPR_POSEGRAPH_BREAKDOWN 2

size_t sgpr_posegraph_optimize_workspace_bytes(int M, int C);

int sgpr_posegraph_optimize(const double* d_X, int M, const int32_t* h_starts, int n_sessions, const int32_t* d_rows,
                            const int32_t* d_cols, const double* d_T, const double* d_weight, int C,
                            const uint8_t* d_fixed, double w_odo_rot, double w_odo_trans, double w_clo_rot,
                            double w_clo_trans, int max_iters, double rel_tol, double* d_X_out, int32_t* d_info,
                            double* d_resid, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGPR_POSEGRAPH_H */
