"""NumPy reference of the path-set score filter (include/sgpr.h, sgpr_seq_path_filter):

    D_p(r, c)    = { d in 0..L-1 : r - d >= 0 and 0 <= c - sigma off_p[d] < M }      (a prefix: off is monotone)
    Q_{p,sigma}  = (S[r, c] + S[r-1, c - sigma off_p[1]] + ...) * rcp[|D_p|],        rcp[n] = float32(1.0 / n)

float32 accumulators, the d loop outermost (so every entry adds its terms in ascending d), one float32 multiplication.
The result folds the candidates - forward paths 0..P-1, then reverse paths 0..P-1 -: best starts as the first one, a later
x replaces it iff x > best or best is NaN; code = direction bit | path << 1 of the winner."""
from fractions import Fraction

import numpy as np

MAX_LEN = 32
MAX_PATHS = 16
MAX_OFFSET = 64
RCP = np.array([0.0] + [1.0 / n for n in range(1, MAX_LEN + 1)], dtype=np.float64).astype(np.float32)
SLOPES = ("1", "1/2", "2/3", "3/2", "2")     # the path set of the planted gates: 9 paths


def seq_paths(seq_len, slopes):
    """one path per slope p/q ((p, q), a Fraction or a string like "3/2") and phase j in 0..q-1, off[d] = (d p + j) // q,
    de-duplicated in order -> int32 [P, seq_len]; ValueError past MAX_PATHS paths or past offset MAX_OFFSET"""
    paths = []
    for s in slopes:
        f = Fraction(*s) if isinstance(s, (tuple, list)) else Fraction(s)
        p, q = f.numerator, f.denominator
        for j in range(q):
            off = [(d * p + j) // q for d in range(seq_len)]
            if off[-1] > MAX_OFFSET:
                raise ValueError("offset %d above %d" % (off[-1], MAX_OFFSET))
            if off not in paths:
                paths.append(off)
    if len(paths) > MAX_PATHS:
        raise ValueError("%d paths: more than %d" % (len(paths), MAX_PATHS))
    return np.asarray(paths, dtype=np.int32).reshape(len(paths), seq_len)


def unit_path(seq_len):
    return np.arange(seq_len, dtype=np.int32)[None, :]


def _one(s, off, sigma):
    """Q_{p,sigma} for every entry of s"""
    r, m = s.shape
    acc = s.copy()
    cnt = np.ones((r, m), dtype=np.int64)
    with np.errstate(all="ignore"):
        for d in range(1, len(off)):
            o = int(off[d])
            if d >= r or o >= m:
                break
            # entries (r, c) with r - d >= 0 and 0 <= c - sigma o < m
            if sigma > 0:
                acc[d:, o:] = acc[d:, o:] + s[:r - d, :m - o]
                cnt[d:, o:] += 1
            else:
                acc[d:, :m - o] = acc[d:, :m - o] + s[:r - d, o:]
                cnt[d:, :m - o] += 1
        return (acc * RCP[cnt]).astype(np.float32)


def path_filter(s, paths, ctx=0, forward=True, reverse=False):
    """-> (Q float32 [R - ctx, M], code uint8 [R - ctx, M])"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    paths = np.asarray(paths, dtype=np.int32)
    assert s.ndim == 2 and paths.ndim == 2 and 1 <= paths.shape[1] <= MAX_LEN and 1 <= paths.shape[0] <= MAX_PATHS
    assert 0 <= ctx <= s.shape[0] and (forward or reverse)
    assert (paths[:, 0] == 0).all() and (np.diff(paths, axis=1) >= 0).all() and paths.max() <= MAX_OFFSET
    best = code = None
    for sigma, bit in ((+1, 0), (-1, 1)):
        if not (forward if sigma > 0 else reverse):
            continue
        for p, off in enumerate(paths):
            x = _one(s, off, sigma)
            c = np.uint8(bit | (p << 1))
            if best is None:
                best, code = x, np.full(s.shape, c, dtype=np.uint8)
                continue
            with np.errstate(invalid="ignore"):
                take = (x > best) | np.isnan(best)
            best, code = np.where(take, x, best), np.where(take, c, code).astype(np.uint8)
    return np.ascontiguousarray(best[ctx:]), np.ascontiguousarray(code[ctx:])


def planted(seed, slope=(1, 1), n=400):
    """seq_ref.planted with a revisit of slope p/q: noise below 0.8; rows 200..299 revisit column ((r - 200) p) // q
    (driven the same way), rows 300..399 column 199 - ((r - 300) p) // q (the opposite way), each planted entry
    0.63 + up to 0.3 -> (S, planted column per row or -1)"""
    p, q = slope
    rng = np.random.default_rng(seed)
    s = rng.random((n, n), dtype=np.float32) * np.float32(0.8)
    col = np.full(n, -1, dtype=np.int64)
    col[200:300] = ((np.arange(200, 300) - 200) * p) // q
    col[300:400] = 199 - ((np.arange(300, 400) - 300) * p) // q
    lift = rng.random(200, dtype=np.float32)
    for i, r in enumerate(range(200, 400)):
        s[r, col[r]] = np.float32(0.45) + np.float32(0.18) + lift[i] * np.float32(0.3)
    return s, col
