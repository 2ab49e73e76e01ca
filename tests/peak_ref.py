"""NumPy reference of distinct-place loop closures (include/sgpr.h, sgpr_peak_filter / sgpr_score_peak_topk):

    a column QUALIFIES for row r iff it is eligible (window, causal, self_r = row_self[r] or row0 + r) and its value is
    neither NaN nor -inf; qualifying columns are ordered by value descending (IEEE comparison: -0.0 ties +0.0), then
    column ascending;
    column c is a PEAK of row r iff it qualifies and comes first, in that order, among the qualifying columns c' with
    |c' - c| <= rho.

Written the slow and obvious way: for each column, a loop over its neighbourhood (`is_peak` one column at a time in
Python; `peaks` the same loop over the neighbourhood's offsets with every column of the matrix compared at once, for the
matrices the GPU tests use - the host tests hold the two to each other).  `lists` is the selection reference: the k best
columns of a matrix in that order, values read back from the matrix at their index (the stored bits), (-inf, -1) in the
slots past the last qualifying column."""
import numpy as np

MAX_RADIUS = 1024


def eligible(r, m, window=-1, row0=0, causal=False, row_self=None):
    """sgpr_score_topk's eligibility -> bool [r, m]: |c - self| > window (window < 0: no window), causal: c < self"""
    own = (np.arange(r, dtype=np.int64) + int(row0)) if row_self is None else np.asarray(row_self, dtype=np.int64)
    assert own.shape == (r,)
    cc = np.arange(m, dtype=np.int64)[None, :]
    ok = np.ones((r, m), dtype=bool)
    if window >= 0:
        ok &= np.abs(cc - own[:, None]) > window
    if causal:
        ok &= cc < own[:, None]
    return ok


def qualifies(x, window=-1, row0=0, causal=False, row_self=None):
    x = np.asarray(x, dtype=np.float32)
    return eligible(x.shape[0], x.shape[1], window, row0, causal, row_self) & ~np.isnan(x) & (x != -np.inf)


def is_peak(row, ok, c, rho):
    """one column of one row, literally: no qualifying column within rho comes before c in the order"""
    if not ok[c]:
        return False
    for j in range(max(0, c - rho), min(len(row), c + rho + 1)):
        if j == c or not ok[j]:
            continue
        if row[j] > row[c] or (row[j] == row[c] and j < c):   # (-0.0 == +0.0)
            return False
    return True


def peaks_slow(x, rho, **elig):
    x = np.asarray(x, dtype=np.float32)
    ok = qualifies(x, **elig)
    return np.array([[is_peak(x[r], ok[r], c, rho) for c in range(x.shape[1])] for r in range(x.shape[0])],
                    dtype=bool).reshape(x.shape)


def peaks(x, rho, **elig):
    """-> bool [R, M]; the loop over the neighbourhood, one offset at a time for all columns at once"""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2 and 0 <= rho <= MAX_RADIUS
    r, m = x.shape
    ok = qualifies(x, **elig)
    peak = ok.copy()
    with np.errstate(invalid="ignore"):
        for d in range(1, min(rho, m - 1) + 1):
            # the neighbour d to the left beats c when it is >= (equal values: the lower column first) ...
            peak[:, d:] &= ~(ok[:, :-d] & (x[:, :-d] >= x[:, d:]))
            # ... the neighbour d to the right only when it is larger
            peak[:, :-d] &= ~(ok[:, d:] & (x[:, d:] > x[:, :-d]))
    return peak


def peak_filter(x, rho, **elig):
    """-> P float32 [R, M]: x (the stored bits) at a peak, -inf elsewhere"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return np.where(peaks(x, rho, **elig), x, np.float32(-np.inf)).astype(np.float32)


def lists(x, k, **elig):
    """the selection reference -> (values float32 [R, k], indices int32 [R, k])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    r, m = x.shape
    vals = np.full((r, k), -np.inf, dtype=np.float32)
    idx = np.full((r, k), -1, dtype=np.int32)
    if m == 0 or r == 0:
        return vals, idx
    ok = qualifies(x, **elig)
    key = np.where(ok, x + np.float32(0.0), np.float32(-np.inf))          # -0.0 as +0.0; what does not qualify last
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]                 # value descending, column ascending
    listed = np.take_along_axis(ok, order, axis=1)
    n = order.shape[1]
    idx[:, :n] = np.where(listed, order, -1)
    vals[:, :n] = np.where(listed, np.take_along_axis(x, order, axis=1), np.float32(-np.inf))
    return vals, idx


def peak_lists(x, rho, k, **elig):
    """the k best peaks of every row in list order -> (values, indices)"""
    return lists(peak_filter(x, rho, **elig), k, **elig)


def places_per_list(idx, rho):
    """mean number of places in a list: groups of listed columns (>= 0) at most rho apart, over the lists that are
    not empty"""
    idx = np.asarray(idx)
    counts = []
    for row in idx:
        c = np.sort(row[row >= 0])
        if c.size:
            counts.append(1 + int((np.diff(c) > rho).sum()))
    return float(np.mean(counts)) if counts else 0.0


def planted(seed=0, m=400):
    """The planted case: one row of noise in [0, 0.01) with three bumps h exp(-d^2 / 50), h = 0.9, 0.8, 0.7, centred on
    columns 100, 200, 300.  A bump loses at least 0.7 (1 - exp(-1 / 50)) = 0.0139 one column from its centre - more than
    the noise can make up."""
    rng = np.random.default_rng(seed)
    x = rng.random((1, m), dtype=np.float32) * np.float32(0.01)
    c = np.arange(m, dtype=np.float64)
    for h, centre in ((0.9, 100), (0.8, 200), (0.7, 300)):
        x[0] += (h * np.exp(-(c - centre) ** 2 / 50.0)).astype(np.float32)
    return x
