"""NumPy reference of pairwise-consistent loop closures (include/sgpr.h, sgpr_closure_consistency / sgpr_consistent_set;
DESIGN.md §24), written from the definitions: float64, every operation a plain ufunc rounded on its own (no einsum, no
dot, nothing a BLAS could fuse), so the GPU results can be compared bit for bit.

An SE(2) element is a row (c, s, x, y) acting as p -> R p + t, R = [[c, -s], [s, c]].
closure_consistency(...) -> (adj int64 [C, ceil(C/64)], degree int32 [C], members int32 [C]);
consistent_set(adj, group, n_groups) -> (rank int32 [C], group_size int32 [n_groups]).
"""
import math

import numpy as np

MAX_CLOSURES = 16384
MAX_GROUPS = 4096


def compose(A, B):
    """A o B (B first) on arrays [..., 4]"""
    ac, as_, ax, ay = A[..., 0], A[..., 1], A[..., 2], A[..., 3]
    bc, bs, bx, by = B[..., 0], B[..., 1], B[..., 2], B[..., 3]
    c = ac * bc - as_ * bs
    s = as_ * bc + ac * bs
    x = (ac * bx - as_ * by) + ax
    y = (as_ * bx + ac * by) + ay
    return np.stack(np.broadcast_arrays(c, s, x, y), axis=-1)


def inverse(A):
    ac, as_, ax, ay = A[..., 0], A[..., 1], A[..., 2], A[..., 3]
    return np.stack((ac, -as_, -(ac * ax + as_ * ay), as_ * ax - ac * ay), axis=-1)


def words_of(C):
    return (int(C) + 63) // 64


def pack_bits(mat):
    """bool [C, C] -> int64 [C, ceil(C/64)], bit q & 63 of word q >> 6"""
    C = mat.shape[0]
    W = words_of(C)
    if C == 0:
        return np.zeros((0, 0), dtype=np.int64)
    wide = np.zeros((C, W * 64), dtype=np.uint8)
    wide[:, :C] = mat
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view("<u8").view(np.int64).reshape(C, W)


def unpack_bits(adj, C):
    """int64 / uint64 [C, W] -> bool [C, C]: bits at or beyond C dropped"""
    if C == 0:
        return np.zeros((0, 0), dtype=bool)
    adj = np.ascontiguousarray(np.asarray(adj)).view(np.uint64).reshape(C, -1)
    return np.unpackbits(adj.view(np.uint8), axis=1, bitorder="little")[:, :C].astype(bool)


def prepare(rows, cols, T, Xr, Xc, group, n_groups):
    """-> G, H, R float64 [C, 4] (garbage but finite-indexed for a void closure) and members int32 [C] = group of every
    non-void closure, -1 for a void one"""
    rows, cols, group = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (rows, cols, group))
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4)
    Xr = np.asarray(Xr, dtype=np.float64).reshape(-1, 4)
    Xc = np.asarray(Xc, dtype=np.float64).reshape(-1, 4)
    ok = (rows >= 0) & (rows < Xr.shape[0]) & (cols >= 0) & (cols < Xc.shape[0]) & (group >= 0) & (group < n_groups)
    Rp = Xr[np.where(ok, rows, 0)] if Xr.shape[0] else np.zeros((rows.size, 4))
    Cp = Xc[np.where(ok, cols, 0)] if Xc.shape[0] else np.zeros((rows.size, 4))
    ok &= np.isfinite(T).all(1) & np.isfinite(Rp).all(1) & np.isfinite(Cp).all(1)
    with np.errstate(all="ignore"):
        G = compose(compose(Cp, T), inverse(Rp))
        H = compose(inverse(T), inverse(Cp))
    return G, H, Rp, np.where(ok, group, -1).astype(np.int32)


def closure_consistency(rows, cols, T, Xr, Xc, group, n_groups, max_trans, min_cos, lever_gain, chunk=512):
    G, H, R, members = prepare(rows, cols, T, Xr, Xc, group, n_groups)
    C = members.size
    upper = np.zeros((C, C), dtype=bool)
    q = np.arange(C)
    max_trans, min_cos, lever_gain = np.float64(max_trans), np.float64(min_cos), np.float64(lever_gain)
    with np.errstate(all="ignore"):
        for p0 in range(0, C, chunk):
            p = np.arange(p0, min(C, p0 + chunk))
            D = compose(compose(H[None, :, :], G[p, None, :]), R[None, :, :])     # [p, q]: (a, b) = (p, q)
            dx = R[None, :, 2] - R[p, None, 2]
            dy = R[None, :, 3] - R[p, None, 3]
            lever = np.sqrt(dx * dx + dy * dy)
            tau = max_trans + lever_gain * lever
            ok = (D[..., 0] >= min_cos) & (D[..., 2] * D[..., 2] + D[..., 3] * D[..., 3] <= tau * tau)
            ok &= (q[None, :] > p[:, None]) & (members[None, :] == members[p, None]) & (members[p, None] >= 0)
            upper[p] = ok
    mat = upper | upper.T
    return pack_bits(mat), mat.sum(1).astype(np.int32), members


def _bits(adj, C):
    mat = unpack_bits(adj, C)
    mat[np.arange(C), np.arange(C)] = False
    return mat


def consistent_set_literal(adj, group, n_groups):
    """the greedy rule exactly as stated: every round recounts every candidate"""
    group = np.asarray(group, dtype=np.int64).reshape(-1)
    C = group.size
    mat = _bits(adj, C)
    rank = np.full(C, -1, dtype=np.int32)
    size = np.zeros(n_groups, dtype=np.int32)
    for g in range(n_groups):
        cand = group == g
        while cand.any():
            d = np.where(cand, (mat & cand[None, :]).sum(1), -1)
            v = int(np.argmax(d))                     # the first maximum: the lowest index
            rank[v] = size[g]
            size[g] += 1
            cand = cand & mat[v]
    return rank, size


def consistent_set(adj, group, n_groups):
    """the same result with the counts updated instead of recounted (what leaves cand is subtracted)"""
    group = np.asarray(group, dtype=np.int64).reshape(-1)
    C = group.size
    mat = _bits(adj, C)
    rank = np.full(C, -1, dtype=np.int32)
    size = np.zeros(n_groups, dtype=np.int32)
    order = np.argsort(group, kind="stable")
    lo = np.searchsorted(group[order], np.arange(n_groups), side="left")
    hi = np.searchsorted(group[order], np.arange(n_groups), side="right")
    for g in range(n_groups):
        m = order[lo[g]:hi[g]]                        # members, ascending
        if m.size == 0:
            continue
        sub = mat[np.ix_(m, m)]
        alive = np.arange(m.size)
        d = sub.sum(1).astype(np.int64)
        while alive.size:
            i = int(np.argmax(d))
            v = alive[i]
            rank[m[v]] = size[g]
            size[g] += 1
            keep = sub[v, alive]
            gone = alive[~keep]
            alive = alive[keep]
            d = d[keep] - sub[np.ix_(alive, gone)].sum(1)
    return rank, size


def consistent_closures(refined, flags, accept, rows, cols, Xr, Xc, row_starts=None, col_starts=None, max_trans=1.0,
                        max_yaw=0.06, lever_gain=0.04, min_clique=3):
    """What SG.consistent_closures computes, on host arrays: refined [P,4], flags [P], accept bool [P] or None,
    rows / cols [P]; Xr / Xc the planar odometry; row_starts / col_starts the first scan of every session (None: one).
    -> dict accept bool [P], rank, degree int32 [P], group_size int32 [n_groups]"""
    rows, cols = np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(cols, dtype=np.int64).reshape(-1)
    rs = np.asarray([0] if row_starts is None else row_starts, dtype=np.int64)
    cs = np.asarray([0] if col_starts is None else col_starts, dtype=np.int64)
    void = (np.asarray(flags).reshape(-1).astype(np.int64) & (1 | 2 | 8)) != 0
    if accept is not None:
        void |= ~np.asarray(accept, dtype=bool).reshape(-1)
    group = (np.searchsorted(rs, rows, side="right") - 1) * cs.size + (np.searchsorted(cs, cols, side="right") - 1)
    group = np.where(void | (rows < 0) | (cols < 0), -1, group)
    n_groups = int(rs.size * cs.size)
    adj, degree, members = closure_consistency(rows, cols, refined, Xr, Xc, group, n_groups, max_trans,
                                               math.cos(max_yaw), lever_gain)
    rank, size = consistent_set(adj, members, n_groups)
    ok = (rank >= 0) & (size[np.where(members >= 0, members, 0)] >= min_clique)
    return {"accept": ok, "rank": rank, "degree": degree, "group_size": size}
