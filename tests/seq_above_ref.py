"""NumPy reference of the range selection on the sequence-matched score (include/sgpr.h, sgpr_seq_rows_above):
seq_ref.seq_filter, then sgpr_score_topk's eligibility rule on the end point and np.nonzero in row-major order."""
import numpy as np

import seq_ref


def eligible(r, m, ctx=0, window=-1, row0=0, causal=False, row_self=None):
    """bool [r - ctx, m]: column c is eligible for row ctx + o iff |c - self| > window (window < 0: no window) and,
    causal, c < self; self = row_self[row] or row0 + row, rows counted over all r"""
    rows = np.arange(ctx, r, dtype=np.int64)
    own = (np.asarray(row_self, dtype=np.int64)[ctx:r] if row_self is not None else row0 + rows)[:, None]
    cc = np.arange(m, dtype=np.int64)[None, :]
    ok = np.ones((r - ctx, m), dtype=bool)
    if window >= 0:
        ok &= np.abs(cc - own) > window
    if causal:
        ok &= cc < own
    return ok


def select(q, d, ok, threshold):
    """the entries of q (with their directions d) that are eligible and >= threshold, row-major
    -> (rows i32, cols i32, values f32, dirs u8, row_ptr i64 [rows + 1]); NaN never qualifies"""
    with np.errstate(invalid="ignore"):
        hit = ok & (q >= np.float32(threshold))
    rows, cols = np.nonzero(hit)
    row_ptr = np.concatenate(([0], np.cumsum(hit.sum(axis=1)))).astype(np.int64)
    return rows.astype(np.int32), cols.astype(np.int32), q[rows, cols], d[rows, cols], row_ptr


def seq_above(s, seq_len, threshold, ctx=0, forward=True, reverse=False, window=-1, row0=0, causal=False, row_self=None):
    q, d = seq_ref.seq_filter(s, seq_len, ctx, forward, reverse)
    r, m = np.asarray(s).shape
    return select(q, d, eligible(r, m, ctx, window, row0, causal, row_self), threshold)
