"""NumPy reference of the diagonal score filter (include/sgpr.h, sgpr_seq_filter):

    D(r, c)     = { d in 0..L-1 : r - d >= 0 and 0 <= c - sigma d < M }
    Q_sigma     = (S[r, c] + S[r-1, c-sigma] + ...) * rcp[|D|],   rcp[n] = float32(1.0 / n)

float32 accumulators, the d loop outermost (so every entry adds its terms in ascending d), one float32 multiplication.
Both directions: reverse where it is larger or forward is NaN, forward wins ties."""
import numpy as np

MAX_LEN = 32
RCP = np.array([0.0] + [1.0 / n for n in range(1, MAX_LEN + 1)], dtype=np.float64).astype(np.float32)


def term_counts(r, m, seq_len, sigma):
    """|D(r, c)| for every entry of an r x m matrix"""
    rr = np.arange(r)[:, None]
    cc = np.arange(m)[None, :]
    edge = cc + 1 if sigma > 0 else m - cc
    return np.minimum(seq_len, np.minimum(rr + 1, edge)).astype(np.int64)


def _one_direction(s, seq_len, sigma):
    r, m = s.shape
    acc = s.copy()
    with np.errstate(all="ignore"):
        for d in range(1, seq_len):
            if d >= r or d >= m:
                break
            # entries (r, c) with r - d >= 0 and 0 <= c - sigma d < m
            if sigma > 0:
                acc[d:, d:] = acc[d:, d:] + s[:r - d, :m - d]
            else:
                acc[d:, :m - d] = acc[d:, :m - d] + s[:r - d, d:]
        return (acc * RCP[term_counts(r, m, seq_len, sigma)]).astype(np.float32)


def seq_filter(s, seq_len, ctx=0, forward=True, reverse=False):
    """-> (Q float32 [R - ctx, M], dir uint8 [R - ctx, M])"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    assert s.ndim == 2 and 1 <= seq_len <= MAX_LEN and 0 <= ctx <= s.shape[0] and (forward or reverse)
    if forward and reverse:
        qf, qr = _one_direction(s, seq_len, +1), _one_direction(s, seq_len, -1)
        with np.errstate(invalid="ignore"):
            take = (qr > qf) | np.isnan(qf)
        q, d = np.where(take, qr, qf), take.astype(np.uint8)
    elif forward:
        q = _one_direction(s, seq_len, +1)
        d = np.zeros(s.shape, dtype=np.uint8)
    else:
        q = _one_direction(s, seq_len, -1)
        d = np.ones(s.shape, dtype=np.uint8)
    return np.ascontiguousarray(q[ctx:]), np.ascontiguousarray(d[ctx:])


def planted(seed, n=400):
    """The planted case: noise below 0.8; rows 200..299 revisit columns r - 200 (driven the same way), rows 300..399
    columns 199 - (r - 300) (the opposite way), each planted entry 0.63 + up to 0.3 -> (S, planted column per row or -1)"""
    rng = np.random.default_rng(seed)
    s = rng.random((n, n), dtype=np.float32) * np.float32(0.8)
    col = np.full(n, -1, dtype=np.int64)
    col[200:300] = np.arange(200, 300) - 200
    col[300:400] = 199 - (np.arange(300, 400) - 300)
    lift = rng.random(200, dtype=np.float32)
    for i, r in enumerate(range(200, 400)):
        s[r, col[r]] = np.float32(0.45) + np.float32(0.18) + lift[i] * np.float32(0.3)
    return s, col


def top1(q, window, row0=0):
    """the best column per row outside |c - (row0 + r)| <= window (lowest column among equals); NaN never wins"""
    r, m = q.shape
    rr = np.arange(r)[:, None] + row0
    cc = np.arange(m)[None, :]
    masked = np.where((np.abs(cc - rr) > window) & ~np.isnan(q), q, -np.inf)
    return masked.argmax(axis=1)


def planted_rates(q, col, window=50, skip=8):
    """fraction of rows whose top-1 is the planted column, for the forward revisit (rows 200 + skip .. 299) and the
    reverse one (300 + skip .. 399)"""
    best = top1(q, window)
    fwd = np.arange(200 + skip, 300)
    rev = np.arange(300 + skip, 400)
    return float(np.mean(best[fwd] == col[fwd])), float(np.mean(best[rev] == col[rev]))
