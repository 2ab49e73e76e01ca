"""NumPy reference of the session-aware path-set filter (include/sgpr.h, sgpr_session_filter):

    sess(x)      = the largest j with starts[j] <= x (x < 0: session 0); lo(x) / hi(x): its first / last index
    D_p(r, c)    = { d in 0..L-1 : r - d >= lo_row(r) and lo_col(c) <= c - sigma off_p[d] <= hi_col(c) }     (a prefix)
    Q_{p,sigma}  = (S[r, c] + S[r-1, c - sigma off_p[1]] + ...) * rcp[|D_p|],        rcp[n] = float32(1.0 / n)

float32 accumulators, the d loop outermost (every entry adds its terms in ascending d), one float32 multiplication; the
fold over the candidates and the code are seq_path_ref.path_filter's.  With window >= 0 the end point (r, c) is excluded
(-inf, code 0) iff sess_col(c) == sess_col(self_r) and |c - self_r| <= window, self_r = row_self[r] or row0 + r."""
import numpy as np

from seq_path_ref import MAX_LEN, MAX_PATHS, MAX_OFFSET, RCP, unit_path

SESSION_MAX = 64


def table(starts, limit):
    """a checked session table (None: one session) -> int64 array"""
    t = np.zeros(1, dtype=np.int64) if starts is None else np.asarray(starts, dtype=np.int64)
    assert t.ndim == 1 and 1 <= len(t) <= SESSION_MAX and t[0] == 0 and (np.diff(t) >= 0).all() and t[-1] <= limit
    return t


def sess(starts, x):
    """session index of every index in x (below 0: session 0; at or past the end: the rule gives the last session)"""
    starts = np.asarray(starts, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64)
    return np.where(x < 0, 0, np.searchsorted(starts, x, side="right") - 1)


def lo(starts, x):
    return np.asarray(starts, dtype=np.int64)[sess(starts, x)]


def hi(starts, x, limit):
    """last index of the session of every x; `limit` is the number of rows / columns"""
    ends = np.append(np.asarray(starts, dtype=np.int64)[1:], limit) - 1
    return ends[sess(starts, x)]


def _one(s, off, sigma, lo_r, lo_c, hi_c):
    r, m = s.shape
    acc = s.copy()
    cnt = np.ones((r, m), dtype=np.int64)
    rr, cc = np.arange(r), np.arange(m)
    with np.errstate(all="ignore"):
        for d in range(1, len(off)):
            src_c = cc - sigma * int(off[d])
            ok = ((rr - d >= lo_r)[:, None]) & ((src_c >= lo_c) & (src_c <= hi_c))[None, :]
            if not ok.any():
                break                                 # a prefix: nothing later is in either
            term = s[np.clip(rr - d, 0, r - 1)][:, np.clip(src_c, 0, m - 1)]
            acc = np.where(ok, acc + term, acc).astype(np.float32)
            cnt += ok
        return (acc * RCP[cnt]).astype(np.float32)


def session_filter(s, paths=None, L=None, ctx=0, forward=True, reverse=False, row_starts=None, col_starts=None,
                   window=-1, row_self=None, row0=0):
    """-> (Q float32 [R - ctx, M], code uint8 [R - ctx, M]); paths None: the unit diagonal of length L"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    paths = unit_path(L) if paths is None else np.asarray(paths, dtype=np.int32)
    assert s.ndim == 2 and paths.ndim == 2 and 1 <= paths.shape[1] <= MAX_LEN and 1 <= paths.shape[0] <= MAX_PATHS
    assert 0 <= ctx <= s.shape[0] and (forward or reverse) and window >= -1
    assert (paths[:, 0] == 0).all() and (np.diff(paths, axis=1) >= 0).all() and paths.max() <= MAX_OFFSET
    r, m = s.shape
    rt, ct = table(row_starts, r), table(col_starts, m)
    lo_r = lo(rt, np.arange(r))
    lo_c, hi_c = lo(ct, np.arange(m)), hi(ct, np.arange(m), m)
    best = code = None
    for sigma, bit in ((+1, 0), (-1, 1)):
        if not (forward if sigma > 0 else reverse):
            continue
        for p, off in enumerate(paths):
            x = _one(s, off, sigma, lo_r, lo_c, hi_c)
            c = np.uint8(bit | (p << 1))
            if best is None:
                best, code = x, np.full(s.shape, c, dtype=np.uint8)
                continue
            with np.errstate(invalid="ignore"):
                take = (x > best) | np.isnan(best)
            best, code = np.where(take, x, best), np.where(take, c, code).astype(np.uint8)
    if window >= 0:
        ex = excluded(r, m, ct, window, row_self, row0)
        best, code = np.where(ex, np.float32(-np.inf), best), np.where(ex, np.uint8(0), code)
    return np.ascontiguousarray(best[ctx:], dtype=np.float32), np.ascontiguousarray(code[ctx:], dtype=np.uint8)


def excluded(r, m, col_starts, window, row_self=None, row0=0):
    """bool [r, m]: the session window (window < 0: nothing)"""
    ct = table(col_starts, m)
    self_r = (row0 + np.arange(r, dtype=np.int64)) if row_self is None else np.asarray(row_self, dtype=np.int64)
    cc = np.arange(m, dtype=np.int64)
    return (sess(ct, cc)[None, :] == sess(ct, self_r)[:, None]) & (np.abs(cc[None, :] - self_r[:, None]) <= window)


def topk(q, k, row_self=None, row0=0, causal=False):
    """sgpr_topk_rows_large without a window on a filtered block: (value descending by IEEE comparison, column
    ascending), NaN and -inf never listed, (-inf, -1) padding -> (values f32 [n, k], indices i32 [n, k])"""
    n, m = q.shape
    vals = np.full((n, k), -np.inf, dtype=np.float32)
    idx = np.full((n, k), -1, dtype=np.int32)
    self_r = (row0 + np.arange(n, dtype=np.int64)) if row_self is None else np.asarray(row_self, dtype=np.int64)
    for i in range(n):
        ok = ~np.isnan(q[i]) & (q[i] != -np.inf)
        if causal:
            ok &= np.arange(m) < self_r[i]
        cols = np.flatnonzero(ok)
        order = cols[np.argsort(-q[i, cols].astype(np.float64), kind="stable")][:k]
        vals[i, :len(order)] = q[i, order]
        idx[i, :len(order)] = order
    return vals, idx


# ------------------------------------------------------------------------------------------------- the planted world
N, SESSION = 450, 150
WORLD_STARTS = np.array([0, 150, 300], dtype=np.int32)


def planted(seed):
    """three sessions of 150 scans, rows and columns: noise below 0.8; session B (rows 150..299) retraces A backwards
    from A's end (column 149 - (r - 150)), session C (rows 300..449) retraces B forwards from B's start (column
    150 + (r - 300)); a planted entry is 0.63 + lift[r] * 0.3 -> (S, planted column per row or -1)"""
    rng = np.random.default_rng(seed)
    s = rng.random((N, N), dtype=np.float32) * np.float32(0.8)
    lift = rng.random(N, dtype=np.float32)
    col = np.full(N, -1, dtype=np.int64)
    col[150:300] = 149 - (np.arange(150, 300) - 150)
    col[300:450] = 150 + (np.arange(300, 450) - 300)
    for r in range(150, 450):
        s[r, col[r]] = np.float32(0.63) + lift[r] * np.float32(0.3)
    return s, col


def planted_groups(L, window=50):
    """rows of "B head" (partner within `window` columns across the seam), "C head" (fewer than L - 1 rows after the
    session start) and "rest" """
    return (np.arange(150, 150 + window // 2), np.arange(300, 300 + L - 1),
            np.concatenate([np.arange(175 + L, 300), np.arange(300 + L, 450)]))


def index_window_top1(q, window):
    """top-1 column per row under today's rule |c - r| > window (-1 where nothing qualifies)"""
    n, m = q.shape
    x = np.where(np.abs(np.arange(m)[None, :] - np.arange(n)[:, None]) <= window, -np.inf, q)
    return topk(x.astype(np.float32), 1)[1][:, 0]


def recall(best, col, rows):
    return float(np.mean(best[rows] == col[rows]))
