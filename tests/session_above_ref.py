"""NumPy reference of the thresholded closures on multi-session maps (include/sgpr.h, sgpr_session_rows_above):

    S, the tables, sess / lo / hi, D_p(r, c), Q_{p,sigma}: session_ref's (float32 accumulators, ascending d, one float32
    multiplication by rcp[|D_p|])
    a candidate (p, sigma) takes part in the fold only when |D_p(r, c)| >= min_terms; the fold visits the participating
    candidates forward before reverse, paths ascending, with q > best or best is NaN, the first of them initialising it;
    an end point with no participating candidate is not eligible
    eligible: not excluded by the session window, causal: c < self_r, and at least one participating candidate
    selected: eligible and Q >= threshold (NaN never), row-major -> seq_above_ref.select's arrays with codes for dirs"""
import numpy as np

import seq_above_ref
import session_ref
from seq_path_ref import MAX_LEN, MAX_OFFSET, MAX_PATHS, RCP, unit_path


def candidate(s, off, sigma, lo_r, lo_c, hi_c):
    """session_ref._one with the term count beside the mean -> (Q f32 [R, M], |D| int64 [R, M])"""
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
            term = s[np.clip(rr - d, 0, max(r - 1, 0))][:, np.clip(src_c, 0, max(m - 1, 0))]
            acc = np.where(ok, acc + term, acc).astype(np.float32)
            cnt += ok
        return (acc * RCP[cnt]).astype(np.float32), cnt


def fold(s, paths=None, L=None, ctx=0, forward=True, reverse=False, row_starts=None, col_starts=None, min_terms=1):
    """-> (Q f32 [R - ctx, M], code u8 [R - ctx, M], have bool [R - ctx, M]); Q and code are 0 where have is False"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    paths = unit_path(L) if paths is None else np.asarray(paths, dtype=np.int32)
    assert s.ndim == 2 and paths.ndim == 2 and 1 <= paths.shape[1] <= MAX_LEN and 1 <= paths.shape[0] <= MAX_PATHS
    assert 0 <= ctx <= s.shape[0] and (forward or reverse) and 1 <= min_terms <= paths.shape[1]
    assert (paths[:, 0] == 0).all() and (np.diff(paths, axis=1) >= 0).all() and paths.max() <= MAX_OFFSET
    r, m = s.shape
    rt, ct = session_ref.table(row_starts, r), session_ref.table(col_starts, m)
    lo_r = session_ref.lo(rt, np.arange(r))
    lo_c, hi_c = session_ref.lo(ct, np.arange(m)), session_ref.hi(ct, np.arange(m), m)
    best = np.zeros((r, m), dtype=np.float32)
    code = np.zeros((r, m), dtype=np.uint8)
    have = np.zeros((r, m), dtype=bool)
    for sigma, bit in ((+1, 0), (-1, 1)):
        if not (forward if sigma > 0 else reverse):
            continue
        for p, off in enumerate(paths):
            x, n = candidate(s, off, sigma, lo_r, lo_c, hi_c)
            with np.errstate(invalid="ignore"):
                take = (n >= min_terms) & (~have | (x > best) | np.isnan(best))
            best = np.where(take, x, best).astype(np.float32)
            code = np.where(take, np.uint8(bit | (p << 1)), code).astype(np.uint8)
            have |= take
    return (np.ascontiguousarray(best[ctx:]), np.ascontiguousarray(code[ctx:]), np.ascontiguousarray(have[ctx:]))


def eligible(r, m, ctx, have, col_starts=None, window=-1, row0=0, causal=False, row_self=None):
    """bool [r - ctx, m]: the three conditions of the contract"""
    ok = have.copy()
    if window >= 0:
        ok &= ~session_ref.excluded(r, m, col_starts, window, row_self, row0)[ctx:]
    if causal:
        ok &= seq_above_ref.eligible(r, m, ctx, -1, row0, True, row_self)
    return ok


def session_above(s, threshold, paths=None, L=None, ctx=0, forward=True, reverse=False, row_starts=None, col_starts=None,
                  min_terms=1, window=-1, row0=0, causal=False, row_self=None):
    """-> (rows i32, cols i32, values f32, codes u8, row_ptr i64 [R - ctx + 1])"""
    q, code, have = fold(s, paths, L, ctx, forward, reverse, row_starts, col_starts, min_terms)
    r, m = np.asarray(s).shape
    ok = eligible(r, m, ctx, have, col_starts, window, row0, causal, row_self)
    return seq_above_ref.select(q, code, ok, threshold)


def cut(result, capacity):
    """what a call with `capacity` writes: the first min(count, capacity) pairs; row_ptr stays exact"""
    rows, cols, vals, codes, row_ptr = result
    return rows[:capacity], cols[:capacity], vals[:capacity], codes[:capacity], row_ptr


def precision_recall(rows, cols, planted_col, ctx=0):
    """accepted pairs against the planted world: (count, precision, recall of the planted pairs)"""
    n = len(rows)
    good = int(np.sum(planted_col[np.asarray(rows, dtype=np.int64) + ctx] == cols))
    total = int(np.sum(planted_col >= 0))
    return n, (good / n if n else 1.0), good / total
