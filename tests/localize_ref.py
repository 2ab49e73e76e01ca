"""NumPy reference of scan localisation (include/sgpr_localize.h, sgpr_localize_scans), written from the
header text: float64, every operation a plain ufunc rounded on its own (no einsum, no dot, no np.sum - nothing that could
fuse or reorder), the sums by the literal halving tree, so the GPU results can be compared bit for bit.

localize(map, cols, T, ...) -> (pose float64 [Q,4], stat int32 [Q,4] = (support, live, winner, flags), spread float64 [Q]).
The keyword switches at their defaults are the definition; each other value is a mutant of it (tests/test_localize_host.py).
"""
import math

import numpy as np

from consistency_ref import compose, inverse

MAX_K = 64
MAX_LEN = 16
NO_HYPOTHESIS = 1
DEGENERATE = 2


def tree_sum(v, P2):
    """S(v): v [..., n <= P2] zero-padded (+0) to P2 and reduced by v[i] + v[i + half], half = P2/2 .. 1"""
    v = np.asarray(v, dtype=np.float64)
    a = np.zeros(v.shape[:-1] + (P2,), dtype=np.float64)
    a[..., :v.shape[-1]] = v
    while a.shape[-1] > 1:
        half = a.shape[-1] // 2
        a = a[..., :half] + a[..., half:]
    return a[..., 0]


def sequential_sum(v, P2):
    v = np.asarray(v, dtype=np.float64)
    acc = np.zeros(v.shape[:-1], dtype=np.float64)
    for h in range(v.shape[-1]):
        acc = acc + v[..., h]
    return acc


def session_lo(Q, starts):
    """the first query of every query's session: starts[sess(i)], sess(i) = the largest j with starts[j] <= i"""
    starts = np.asarray([0] if starts is None else starts, dtype=np.int64).reshape(-1)
    return starts[np.searchsorted(starts, np.arange(Q), side="right") - 1]


def hypotheses(map_poses, cols, T, accept=None, odo=None, starts=None, L=1, transport_left=False):
    """-> P float64 [Q, L K, 4] (garbage at a dead slot) and live bool [Q, L K]"""
    map_poses = np.asarray(map_poses, dtype=np.float64).reshape(-1, 4)
    cols = np.asarray(cols, dtype=np.int64)
    Q, K = cols.shape
    T = np.asarray(T, dtype=np.float64).reshape(Q, K, 4)
    M = map_poses.shape[0]
    acc = np.ones((Q, K), dtype=bool) if accept is None else np.asarray(accept).reshape(Q, K) != 0
    lo = session_lo(Q, starts)
    i = np.arange(Q)
    P = np.zeros((Q, L * K, 4), dtype=np.float64)
    live = np.zeros((Q, L * K), dtype=bool)
    padded = np.concatenate((map_poses, np.zeros((1, 4))))
    with np.errstate(all="ignore"):
        for l in range(L):
            j = i - l
            ok = j >= lo
            jj = np.where(ok, j, 0)
            col = cols[jj]                                                  # [Q, K]
            inside = (col >= 0) & (col < M)
            H = compose(padded[np.where(inside, col, M)], T[jj])
            if l > 0:
                od = np.asarray(odo, dtype=np.float64).reshape(Q, 4)
                rel = compose(inverse(od[jj]), od)                          # [Q, 4]
                H = compose(rel[:, None, :], H) if transport_left else compose(H, rel[:, None, :])
            P[:, l * K:(l + 1) * K] = H
            live[:, l * K:(l + 1) * K] = ok[:, None] & inside & acc[jj] & np.isfinite(H).all(-1)
    return P, live


def localize(map_poses, cols, T, accept=None, odo=None, starts=None, L=1, max_trans=1.0, min_cos=math.cos(0.1),
             tree=True, transport_left=False, test_self=False, ties_high=False, only=None):
    """only: the queries to answer (None: all); the rows of the others stay NaN / 0 (a tool checking a sample)"""
    cols = np.asarray(cols)
    Q, K = cols.shape
    assert 1 <= K <= MAX_K and 1 <= L <= MAX_LEN
    P, live = hypotheses(map_poses, cols, T, accept, odo, starts, L, transport_left)
    LK = L * K
    P2 = 1
    while P2 < LK:
        P2 *= 2
    S = tree_sum if tree else sequential_sum
    max_trans, min_cos = np.float64(max_trans), np.float64(min_cos)
    tau2 = max_trans * max_trans
    pose = np.full((Q, 4), np.nan)
    stat = np.zeros((Q, 4), dtype=np.int32)
    spread = np.full(Q, np.nan)
    eye = np.eye(LK, dtype=bool)
    with np.errstate(all="ignore"):
        for i in (range(Q) if only is None else only):
            lv = live[i]
            if not lv.any():
                stat[i] = (0, 0, -1, NO_HYPOTHESIS)
                continue
            p = np.where(lv[:, None], P[i], 0.0)                             # dead slots: defined, never counted
            c, s, x, y = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
            dot = c[:, None] * c[None, :] + s[:, None] * s[None, :]
            dx = x[:, None] - x[None, :]
            dy = y[:, None] - y[None, :]
            agree = (dot >= min_cos) & (dx * dx + dy * dy <= tau2) & lv[:, None] & lv[None, :]
            if test_self:
                support = agree.sum(1)                                       # the mutant: a slot must agree with itself
            else:
                support = 1 + (agree & ~eye).sum(1)
            support = np.where(lv, support, -1)
            best = support.max()
            cand = np.flatnonzero(support == best)
            w = int(cand[-1] if ties_high else cand[0])
            sup = agree[w] & lv
            sup[w] = True
            n = np.float64(int(best))
            sc, ss = S(np.where(sup, c, 0.0), P2), S(np.where(sup, s, 0.0), P2)
            nrm = np.sqrt(sc * sc + ss * ss)
            flags = 0
            if np.isfinite(nrm) and nrm > 0.0:
                g = (sc / nrm, ss / nrm)
            else:
                g = (c[w], s[w])
                flags = DEGENERATE
            tx, ty = S(np.where(sup, x, 0.0), P2) / n, S(np.where(sup, y, 0.0), P2) / n
            ex, ey = x - tx, y - ty
            spread[i] = np.sqrt(S(np.where(sup, ex * ex + ey * ey, 0.0), P2) / n)
            pose[i] = (g[0], g[1], tx, ty)
            stat[i] = (int(best), int(lv.sum()), w, flags)
    return pose, stat, spread


def localize_verified(refined, flags, accept, cols, map_poses, odo=None, starts=None, L=1, max_trans=1.0, max_yaw=0.1,
                      min_support=3):
    """What SG.localize computes, on host arrays: refined [Q,K,4], flags [Q,K], accept bool [Q,K] or None.
    -> dict pose, support, live, winner, flags, spread, accept"""
    void = (np.asarray(flags).astype(np.int64) & (1 | 2 | 8)) != 0
    if accept is not None:
        void |= ~np.asarray(accept, dtype=bool)
    pose, stat, spread = localize(map_poses, cols, refined, ~void, odo, starts, L, max_trans, math.cos(float(max_yaw)))
    return {"pose": pose, "support": stat[:, 0], "live": stat[:, 1], "winner": stat[:, 2], "flags": stat[:, 3],
            "spread": spread, "accept": stat[:, 0] >= int(min_support)}
