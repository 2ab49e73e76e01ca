"""PR / ROC / F1-max of the evaluation loop (eval_batch.py:48-49, 69, 85-87) in numpy.

Same definitions as the sklearn functions the reference calls
(`precision_recall_curve`, `roc_curve`, `auc`); float64 throughout.
"""
import numpy as np


def _binary_clf_curve(gt, score):
    gt = np.asarray(gt, dtype=np.float64).ravel()
    score = np.asarray(score).ravel()
    if gt.size != score.size:
        raise ValueError("gt and score differ in length")
    order = np.argsort(score, kind="mergesort")[::-1]
    s, y = score[order], gt[order]
    ends = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y)[ends]
    fps = 1 + ends - tps
    return fps, tps, s[ends]


def precision_recall_curve(gt, score):
    fps, tps, thr = _binary_clf_curve(gt, score)
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=(ps != 0))
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    return np.hstack((precision[::-1], 1.0)), np.hstack((recall[::-1], 0.0)), thr[::-1]


def f1_max(gt, score):
    """eval_batch.py:85-87: F1 = 2PR/(P+R), nan_to_num, max."""
    p, r, _ = precision_recall_curve(gt, score)
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = 2 * p * r / (p + r)
    return float(np.max(np.nan_to_num(f1)))


def roc_curve(gt, score, drop_intermediate=True):
    """eval_batch.py:48: sklearn.metrics.roc_curve's definition -> (fpr, tpr, thresholds).  Collinear points are
    dropped like sklearn's default does; the first point is (0, 0) at threshold +inf."""
    fps, tps, thr = _binary_clf_curve(gt, score)
    if drop_intermediate and fps.size > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    fps = np.r_[0.0, fps]
    tps = np.r_[0.0, tps]
    thr = np.r_[np.inf, thr]
    fpr = fps / fps[-1] if fps[-1] > 0 else np.full(fps.shape, np.nan)
    tpr = tps / tps[-1] if tps[-1] > 0 else np.full(tps.shape, np.nan)
    return fpr, tpr, thr


def auc(x, y):
    """sklearn.metrics.auc for a monotone x: trapezoidal area (eval_batch.py:49)."""
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    return float(trapezoid(y, x))


def roc_auc(gt, score):
    """eval_batch.py:48-49: area under the ROC curve (dropping collinear points does not change it)."""
    fpr, tpr, _ = roc_curve(gt, score, drop_intermediate=False)
    if np.isnan(fpr).any() or np.isnan(tpr).any():
        return float("nan")
    return auc(fpr, tpr)


# ---------------------------------------------------------------------------------------------------------------------
# Device-side F1-max and ROC area: exact, without sorting the matrix.
#
# F1(t) = 2 TP / (TP + P + FP) can only peak at a threshold t that is the score of a POSITIVE pair (moving t down to a
# negative-only value adds false positives and nothing else), and positives are rare (loop closures).  So the engine
# hands over the scores of the positive pairs (sgpr_pair_positives); their sorted distinct values u[0..U) give TP(>= u[i])
# at once, and one streaming pass over the matrix (sgpr_pair_threshold_counts) counts the negatives between up to 8191
# thresholds: every S-th distinct value gets its exact FP, the S - 1 values between two thresholds a bound (FP is at
# least that of the next threshold).  Segments whose bound beats the best exact F1 are settled by a second pass that
# takes their values as thresholds.  The same first pass ranks every negative among all u (Mann-Whitney):
# AUC = (#{pos > neg} + #{pos == neg} / 2) / (P N), which is sklearn's trapezoid area, ties included.
# `count_fn(thresholds, rank)` -> (int64 [T + 1] negatives with exactly b thresholds <= score, rank_sum or None);
# rank = (u, S, above) asks for rank_sum = sum over negatives of 2 #{positive pairs > s} + #{positive pairs == s}.
MAX_THRESHOLDS = 8191


def _f1(tp, fp, pos):
    tp = np.asarray(tp, dtype=np.float64)
    fp = np.asarray(fp, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
        r = tp / pos if pos > 0 else np.ones_like(tp)
        f = 2 * p * r / (p + r)
    return np.nan_to_num(f)


def distinct_counts(pos_scores):
    """Ascending distinct values of the positive scores and how many pairs carry each."""
    u, mult = np.unique(np.asarray(pos_scores, dtype=np.float32).ravel(), return_counts=True)
    return u, mult.astype(np.int64)


def pr_roc_from_counts(pos_scores, count_fn, want_auc=True, max_thresholds=MAX_THRESHOLDS, distinct=None, refine=True):
    """(F1-max of eval_batch.py:85-87, ROC area of eval_batch.py:48-49, counting passes) from the scores of the
    positive pairs (or `distinct` = their ascending distinct values and multiplicities) and a counting function over
    the negatives (see above).  Without positives F1-max is 0 and the area NaN, like the sorted path (metrics.f1_max /
    roc_auc).  refine=False stops after the first pass (the area is exact then, F1-max a lower bound)."""
    u, mult = distinct if distinct is not None else distinct_counts(pos_scores)
    n_u, p_all = int(u.size), int(mult.sum())
    if n_u == 0:
        return 0.0, float("nan"), 0
    above = np.concatenate((np.cumsum(mult[::-1])[::-1], [0])).astype(np.int64)   # positive pairs with value >= u[i]
    # interval = values [lo, hi) whose FP is not known yet, with a lower bound of it (the exact FP of value hi, 0 past
    # the end); F1 inside it is at most F1(TP(>= u[lo]), that bound).  A pass takes whole intervals as thresholds, best
    # bound first, as many as fit - or, when the best one alone exceeds the budget, as the initial [0, U) may, every
    # stride-th value of it, which leaves the values in between as new intervals.
    ilo, ihi, ifp = np.array([0]), np.array([n_u]), np.array([0])
    best, auc, neg, passes = -1.0, float("nan"), None, 0
    while True:
        bound = _f1(above[ilo], ifp, p_all)
        keep = bound > best
        if not keep.any():
            break
        ilo, ihi, ifp, bound = ilo[keep], ihi[keep], ifp[keep], bound[keep]
        order = np.argsort(-bound, kind="stable")
        ilo, ihi, ifp = ilo[order], ihi[order], ifp[order]
        lens = ihi - ilo
        ntake = int(np.searchsorted(np.cumsum(lens), max_thresholds, side="right"))
        if ntake == 0:                                                   # the best interval alone is too long: sample it
            fine = np.arange(ilo[0], ihi[0], -(-int(lens[0]) // max_thresholds))
        else:
            ln = lens[:ntake]
            fine = np.sort(np.repeat(ilo[:ntake] - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum())))
        rank = None
        if passes == 0 and want_auc:                                     # the first pass samples [0, U) from 0
            rank = (u, int(fine[1] - fine[0]) if fine.size > 1 else n_u, above)
        counts, rank_sum = count_fn(u[fine], rank)
        counts = np.asarray(counts, dtype=np.int64)
        passes += 1
        if neg is None:
            neg = int(counts.sum())
            if rank is not None and neg > 0:
                auc = float(rank_sum) / (2.0 * p_all * neg)
        fp = neg - np.cumsum(counts)[:-1]                                # FP(score >= u[fine[q]]), exact
        best = max(best, float(_f1(above[fine], fp, p_all).max()))
        if ntake == 0:                                                   # the gaps of the sampled interval stay open
            g_lo = np.concatenate(([ilo[0]], fine + 1))
            g_hi = np.concatenate((fine, [ihi[0]]))
            g_fp = np.concatenate((fp, [ifp[0]]))
            open_ = g_hi > g_lo
            ilo = np.concatenate((ilo[1:], g_lo[open_]))
            ihi = np.concatenate((ihi[1:], g_hi[open_]))
            ifp = np.concatenate((ifp[1:], g_fp[open_]))
        else:
            ilo, ihi, ifp = ilo[ntake:], ihi[ntake:], ifp[ntake:]
        if ilo.size == 0 or not refine:
            break
    return max(best, 0.0), auc, passes


def _device_fns(engine, score, pose_xz, p_thresh, n_thresh, gt, row0, distinct=True, to_host=True):
    """(positive scores of the rectangle - as (distinct values, multiplicities), sorted and counted on the device, or
    as the raw float32 list for distinct=False (left on the device for to_host=False: the sharded job all-gathers it
    there) - and the counting function over its negatives)."""
    def count_fn(thresholds, rank):
        counts, bad, rank_sum = engine.pair_threshold_counts(score, thresholds, row0=row0, pose_xz=pose_xz, d_pos=p_thresh,
                                                             d_neg=n_thresh, gt=gt, rank=rank)
        if bad:
            raise ValueError("%d scores are negative or NaN" % bad)
        return counts, rank_sum
    pos, bad = engine.pair_positives(score, row0=row0, pose_xz=pose_xz, d_pos=p_thresh, d_neg=n_thresh, gt=gt)
    if bad:
        raise ValueError("%d scores are negative or NaN" % bad)
    if not distinct:
        return (pos.cpu().numpy() if to_host else pos), count_fn
    import torch
    u, mult = torch.unique(pos, sorted=True, return_counts=True)
    return (u.cpu().numpy(), mult.cpu().numpy().astype(np.int64)), count_fn


def pr_roc_device(engine, score, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None, row0=0, want_auc=True, refine=True):
    """(F1-max, ROC area, counting passes) of a score rectangle that stays on the device.  Ground truth from planar
    poses [M,2] (distance <= p_thresh positive, >= n_thresh negative, in between ignored) or explicit int8 labels
    (1 / 0 / -1)."""
    distinct, count_fn = _device_fns(engine, score, pose_xz, p_thresh, n_thresh, gt, row0)
    return pr_roc_from_counts(None, count_fn, want_auc=want_auc, distinct=distinct, refine=refine)


def f1_max_device(engine, score, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None, row0=0, one_call=True):
    """F1-max of a score rectangle that stays on the device -> (f1_max, counting passes).
    one_call (default): the engine's single entry point (sgpr_f1_max: positives, thresholds, counting passes and the
    F1 reduction all on the device, one small copy at the end); rectangles it reports as too large for that path - more
    than 2^20 positive pairs, more than 4095 values to settle in the second pass - and one_call=False take the multi-call
    path (pr_roc_device), which handles any size.  Both are exact."""
    if one_call and hasattr(engine, "f1_max"):
        res = engine.f1_max(score, row0=row0, pose_xz=pose_xz, d_pos=p_thresh, d_neg=n_thresh, gt=gt)
        status = int(res[1])
        if status == 2:
            raise ValueError("scores of labelled pairs are negative or NaN")
        if status == 0:
            return float(res[0]), int(res[4])
    f1, _, passes = pr_roc_device(engine, score, pose_xz, p_thresh, n_thresh, gt, row0, want_auc=False)
    return f1, passes


def roc_auc_device(engine, score, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None, row0=0):
    """ROC area (eval_batch.py:48-49) of a score rectangle that stays on the device: exact, one counting pass."""
    return pr_roc_device(engine, score, pose_xz, p_thresh, n_thresh, gt, row0, refine=False)[1]


def _pooled_fns(engine, pooled_rows, pooled_cols, pose_xz, p_thresh, n_thresh, gt, row0, distinct=True, to_host=True):
    """_device_fns with the matrix-free producers (Engine.score_positives / score_threshold_counts): the pairs of
    pooled_rows x pooled_cols are scored as they are counted and never stored."""
    def count_fn(thresholds, rank):
        counts, bad, rank_sum = engine.score_threshold_counts(pooled_rows, pooled_cols, thresholds, row0=row0,
                                                              pose_xz=pose_xz, d_pos=p_thresh, d_neg=n_thresh, gt=gt,
                                                              rank=rank)
        if bad:
            raise ValueError("%d scores are negative or NaN" % bad)
        return counts, rank_sum
    pos, bad = engine.score_positives(pooled_rows, pooled_cols, row0=row0, pose_xz=pose_xz, d_pos=p_thresh,
                                      d_neg=n_thresh, gt=gt)
    if bad:
        raise ValueError("%d scores are negative or NaN" % bad)
    if not distinct:
        return (pos.cpu().numpy() if to_host else pos), count_fn
    import torch
    u, mult = torch.unique(pos, sorted=True, return_counts=True)
    return (u.cpu().numpy(), mult.cpu().numpy().astype(np.int64)), count_fn


def pr_roc_pooled(engine, pooled_rows, pooled_cols, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None, row0=0,
                  want_auc=True, refine=True, max_thresholds=None):
    """(F1-max, ROC area, counting passes) of the pairs pooled_rows x pooled_cols WITHOUT the score matrix: pr_roc_device
    with producers that score the pairs as they count them.  The same counts reach the same host code, so F1 and the
    area equal pr_roc_device's on the matrix exactly; a pass takes at most max_thresholds (default: the engine's
    MAX_POOLED_THRESHOLDS) thresholds, so refining F1 may take more passes than on the matrix."""
    if max_thresholds is None:
        max_thresholds = getattr(engine, "MAX_POOLED_THRESHOLDS", MAX_THRESHOLDS)
    distinct, count_fn = _pooled_fns(engine, pooled_rows, pooled_cols, pose_xz, p_thresh, n_thresh, gt, row0)
    return pr_roc_from_counts(None, count_fn, want_auc=want_auc, max_thresholds=max_thresholds, distinct=distinct,
                              refine=refine)


def f1_max_pooled(engine, pooled_rows, pooled_cols, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None, row0=0):
    """F1-max of the pairs pooled_rows x pooled_cols without the score matrix -> (f1_max, counting passes)."""
    f1, _, passes = pr_roc_pooled(engine, pooled_rows, pooled_cols, pose_xz, p_thresh, n_thresh, gt, row0, want_auc=False)
    return f1, passes


def roc_auc_pooled(engine, pooled_rows, pooled_cols, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None, row0=0):
    """ROC area of the pairs pooled_rows x pooled_cols without the score matrix: exact, one counting pass."""
    return pr_roc_pooled(engine, pooled_rows, pooled_cols, pose_xz, p_thresh, n_thresh, gt, row0, refine=False)[1]


def _seq_pooled_fns(engine, pooled_rows, pooled_cols, seq_len, pose_xz, p_thresh, n_thresh, gt, row0, context, reverse,
                    distinct=True, to_host=True):
    """_pooled_fns on the sequence-matched score (Engine.score_seq_positives / score_seq_threshold_counts): rows and
    columns are consecutive scans, the first `context` rows serve as context only."""
    kw = dict(row0=row0, pose_xz=pose_xz, d_pos=p_thresh, d_neg=n_thresh, gt=gt, context=context, reverse=reverse)

    def count_fn(thresholds, rank):
        counts, bad, rank_sum = engine.score_seq_threshold_counts(pooled_rows, pooled_cols, seq_len, thresholds, rank=rank,
                                                                  **kw)
        if bad:
            raise ValueError("%d scores are negative or NaN" % bad)
        return counts, rank_sum
    pos, bad = engine.score_seq_positives(pooled_rows, pooled_cols, seq_len, **kw)
    if bad:
        raise ValueError("%d scores are negative or NaN" % bad)
    if not distinct:
        return (pos.cpu().numpy() if to_host else pos), count_fn
    import torch
    u, mult = torch.unique(pos, sorted=True, return_counts=True)
    return (u.cpu().numpy(), mult.cpu().numpy().astype(np.int64)), count_fn


def pr_roc_seq_pooled(engine, pooled_rows, pooled_cols, seq_len, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None,
                      row0=0, context=0, reverse="both", want_auc=True, refine=True, max_thresholds=None):
    """(F1-max, ROC area, counting passes) of the sequence-matched score of the pairs pooled_rows x pooled_cols (rows
    context .. R-1; Engine.seq_filter's definition) WITHOUT the score matrix or the filtered one: pr_roc_pooled's host
    code over producers that filter each 64 MB row block as they count it.  Equal to pr_roc_device on
    seq_filter(score_all_pairs(...)) exactly.  The row pose of output row o is pose_xz[row0 + context + o]; gt is
    [R - context, M]."""
    if max_thresholds is None:
        max_thresholds = getattr(engine, "MAX_POOLED_THRESHOLDS", MAX_THRESHOLDS)
    distinct, count_fn = _seq_pooled_fns(engine, pooled_rows, pooled_cols, seq_len, pose_xz, p_thresh, n_thresh, gt, row0,
                                         context, reverse)
    return pr_roc_from_counts(None, count_fn, want_auc=want_auc, max_thresholds=max_thresholds, distinct=distinct,
                              refine=refine)


def f1_max_seq_pooled(engine, pooled_rows, pooled_cols, seq_len, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None,
                      row0=0, context=0, reverse="both"):
    """F1-max of the sequence-matched score without any matrix -> (f1_max, counting passes)."""
    f1, _, passes = pr_roc_seq_pooled(engine, pooled_rows, pooled_cols, seq_len, pose_xz, p_thresh, n_thresh, gt, row0,
                                      context, reverse, want_auc=False)
    return f1, passes


def roc_auc_seq_pooled(engine, pooled_rows, pooled_cols, seq_len, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None,
                       row0=0, context=0, reverse="both"):
    """ROC area of the sequence-matched score without any matrix: exact, one counting pass."""
    return pr_roc_seq_pooled(engine, pooled_rows, pooled_cols, seq_len, pose_xz, p_thresh, n_thresh, gt, row0, context,
                             reverse, refine=False)[1]


def counts_of(score, gt):
    """numpy stand-ins for sgpr_pair_positives / sgpr_pair_threshold_counts (tests, small inputs): gt 1 / 0 / negative
    = ignored.  Returns (positive scores, count_fn)."""
    sc = np.ascontiguousarray(score, dtype=np.float32).ravel()
    cls = np.asarray(gt).ravel().astype(np.int64)
    pos, negs = sc[cls > 0], np.sort(sc[cls == 0])

    def count_fn(thresholds, rank):
        thr = np.asarray(thresholds, dtype=np.float32)
        b = np.searchsorted(thr, negs, side="right")                    # thresholds <= score
        counts = np.bincount(b, minlength=thr.size + 1).astype(np.int64)
        rank_sum = None
        if rank is not None:
            u, _, above = rank
            le = np.searchsorted(u, negs, side="right")
            gt_s = above[le]
            eq_s = np.where((le > 0) & (u[np.maximum(le, 1) - 1] == negs), above[np.maximum(le, 1) - 1] - gt_s, 0)
            rank_sum = int((2 * gt_s + eq_s).sum())
        return counts, rank_sum
    return pos, count_fn


def recall_at_n(indices, pose_xz, p_thresh=3.0, window=50, causal=False, chunk=1024, col_starts=None, row_mask=None):
    """Recall@1..K of loop-closure candidates (sgpr_score_topk's indices [M,K] of query frames 0..M-1 against frames
    0..M'-1; -1 = no candidate).  A query counts only if some frame it was allowed to match (|c - r| > window, window < 0:
    no window; causal: c < r) lies within p_thresh of it; it is a hit at N if one of its first N indices does.
    pose_xz: [M', 2] (or [M', 12] KITTI rows).  Plain torch on the indices' device, chunked by rows (not a hot path).
    col_starts (the first frame of every session of a multi-session map, sgpr_session_filter's table): the allowed-match
    rule uses the session window - a frame of another session than the query's is never window-excluded.
    row_mask (bool [M]): only these queries are counted.
    -> float64 numpy [K]: hits at N / counted queries (0 when no query counts)."""
    import torch
    from .allpairs import pose_xz as _xz
    idx = torch.as_tensor(indices)
    dev = idx.device
    xz = _xz(pose_xz).to(dev)
    m, kk = idx.shape
    cols = torch.arange(xz.shape[0], device=dev)
    if col_starts is not None:
        starts = torch.as_tensor(np.asarray(col_starts, dtype=np.int64), device=dev)
        col_sess = torch.searchsorted(starts, cols, right=True) - 1
    hits = torch.zeros(kk, dtype=torch.float64, device=dev)
    counted = 0
    for lo in range(0, m, chunk):
        hi = min(m, lo + chunk)
        rows = torch.arange(lo, hi, device=dev)
        near = torch.cdist(xz[lo:hi], xz) <= p_thresh                        # [n, M']
        ok = torch.ones_like(near)
        if window >= 0 and col_starts is not None:
            row_sess = torch.searchsorted(starts, rows, right=True) - 1
            ok &= ((cols[None, :] - rows[:, None]).abs() > window) | (col_sess[None, :] != row_sess[:, None])
        elif window >= 0:
            ok &= (cols[None, :] - rows[:, None]).abs() > window
        if causal:
            ok &= cols[None, :] < rows[:, None]
        valid = (near & ok).any(dim=1)                                       # queries with a revisit to find
        if row_mask is not None:
            valid &= torch.as_tensor(np.asarray(row_mask, dtype=bool)[lo:hi], device=dev)
        ix = idx[lo:hi].long()
        got = torch.zeros(ix.shape, dtype=torch.bool, device=dev)
        has = ix >= 0
        got[has] = near.gather(1, ix.clamp(min=0))[has]
        first = torch.cummax(got.to(torch.int32), dim=1).values.bool()       # hit within the first N
        hits += (first & valid[:, None]).sum(dim=0).to(torch.float64)
        counted += int(valid.sum())
    return (hits / counted).cpu().numpy() if counted else np.zeros(kk)


def places_per_list(indices, radius):
    """Mean number of distinct places in a candidate list: the listed columns (>= 0) of a row, sorted, fall into groups
    whose neighbours are at most `radius` apart - one place seen several times; averaged over the lists that are not
    empty (0 when all are).  indices [M, K] as every loop-closure call returns them."""
    import torch
    idx = torch.as_tensor(indices).long()
    if idx.numel() == 0:
        return 0.0
    srt = torch.sort(torch.where(idx >= 0, idx, torch.full_like(idx, -1)), dim=1).values     # padding first
    listed = srt >= 0
    gaps = (srt[:, 1:] - srt[:, :-1] > int(radius)) & listed[:, :-1] & listed[:, 1:]
    places = gaps.sum(dim=1) + 1
    some = listed.any(dim=1)
    return float(places[some].double().mean()) if bool(some.any()) else 0.0


def recall_percent_n(num_frames, percent=1.0):
    """Candidates per query of recall@percent (PointNetVLAD): N = max(1, round(M' * percent / 100)), M' database frames."""
    return max(1, int(round(num_frames * float(percent) / 100.0)))


def recall_at_percent(indices, pose_xz, percent=1.0, p_thresh=3.0, window=50, causal=False):
    """Recall@percent of loop-closure candidates: recall_at_n at N = max(1, round(M' * percent / 100)) candidates per
    query, M' = len(pose_xz) database frames.  indices [M, K] with K >= N (ValueError otherwise).  -> (recall, N)."""
    import torch
    from .allpairs import pose_xz as _xz
    idx = torch.as_tensor(indices)
    n = recall_percent_n(_xz(pose_xz).shape[0], percent)
    if idx.dim() != 2 or idx.shape[1] < n:
        raise ValueError("recall@%g%% needs %d candidates per query, indices hold %s" % (percent, n, tuple(idx.shape)))
    return float(recall_at_n(idx[:, :n], pose_xz, p_thresh=p_thresh, window=window, causal=causal)[n - 1]), n


def precision_recall_at(rows, cols, pose_xz, p_thresh=3.0, n_thresh=20.0, window=50, causal=False, chunk=None,
                        col_starts=None):
    """Precision and recall of a list of accepted pairs (sgpr_score_above's rows / cols of query frames 0..M-1 against
    frames 0..M-1, M = len(pose_xz)) under the repository's pair classes: distance <= p_thresh positive, >= n_thresh
    negative, in between not counted.  precision = positives / (positives + negatives) among the pairs; recall =
    positives among the pairs / every eligible positive pair (|c - r| > window, window < 0: no window; causal: c < r),
    counted with plain torch on the poses, chunked by rows (not a hot path).  Distances are compared squared, in float64.
    pose_xz: [M, 2] (or [M, 12] KITTI rows).  col_starts (the first frame of every session of a multi-session map):
    the eligible positives follow the session window, as recall_at_n's - a frame of another session than the query's is
    never window-excluded.  -> (precision, recall) floats, 0 where the denominator is 0."""
    import torch
    from .allpairs import pose_xz as _xz
    rows = torch.as_tensor(rows).long()
    cols = torch.as_tensor(cols).long().to(rows.device)
    xz = _xz(pose_xz).to(device=rows.device, dtype=torch.float64)
    m = xz.shape[0]
    p2, n2 = float(p_thresh) ** 2, float(n_thresh) ** 2
    d2 = ((xz[rows] - xz[cols]) ** 2).sum(dim=1)
    tp = int((d2 <= p2).sum())
    fp = int((d2 >= n2).sum())
    chunk = chunk or max(1, (1 << 24) // max(m, 1))
    allc = torch.arange(m, device=xz.device)
    if col_starts is not None:
        starts = torch.as_tensor(np.asarray(col_starts, dtype=np.int64), device=xz.device)
        col_sess = torch.searchsorted(starts, allc, right=True) - 1
    positives = 0
    for lo in range(0, m, chunk):
        hi = min(m, lo + chunk)
        r = torch.arange(lo, hi, device=xz.device)
        near = ((xz[lo:hi, None, :] - xz[None, :, :]) ** 2).sum(dim=2) <= p2
        if window >= 0 and col_starts is not None:
            near &= ((allc[None, :] - r[:, None]).abs() > window) | (col_sess[None, :] != col_sess[lo:hi, None])
        elif window >= 0:
            near &= (allc[None, :] - r[:, None]).abs() > window
        if causal:
            near &= allc[None, :] < r[:, None]
        positives += int(near.sum())
    precision = tp / (tp + fp) if tp + fp else 0.0
    recall = tp / positives if positives else 0.0
    return precision, recall


def planar_odometry(poses12):
    """KITTI 3x4 pose rows [M, 12] (synth.world_sequence, the graph store) -> float64 [M, 4] planar poses (c, s, x, y)
    under the conventions of closure_pose_errors: heading = atan2(p[2], p[0]), x = p[3], y = p[11].  Each maps a point of
    its scan (x forward, y left) into the sequence's own frame, so the true closure of a pair is
    inverse(X[col]) o X[row] - what SG.consistent_closures and engine.closure_consistency take as odometry."""
    p = np.asarray(poses12.detach().cpu().numpy() if hasattr(poses12, "detach") else poses12, dtype=np.float64).reshape(-1, 12)
    head = np.arctan2(p[:, 2], p[:, 0])
    return np.ascontiguousarray(np.stack((np.cos(head), np.sin(head), p[:, 3], p[:, 11]), axis=1))


def closure_pose_errors(results, rows, cols, poses):
    """Yaw and translation error of verified closures (engine.verify_pairs / SG.verify_closures) against ground-truth
    poses.  results: the dict of fields (or anything with "refined" [..., 4] = c, s, tx, ty and "flags"), rows / cols:
    the row and column frame of every pair, same leading shape; poses [M, 12]: KITTI 3x4 rows as synth.world_sequence
    and the graph store hold them - x = p[3], z = p[11], and the sensor's x axis (forward; y is left) points along
    (p[0], p[2]) in the world's (x, z) plane.  The refined transform maps a point of the row scan into the column scan:
    b = R(yaw) a + t, so the truth is yaw = heading(row) - heading(col), t = R(-heading(col)) (xz(row) - xz(col)).
    A pair without a transform (flags INVALID_INDEX / NO_HYPOTHESIS / NONFINITE) gets NaN errors.
    -> dict: yaw_deg, trans_m (float64 numpy, the pairs' shape), median_yaw_deg, median_trans_m (NaN-ignoring; NaN when
    no pair has a transform)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    ref = host(results["refined"]).astype(np.float64)
    flags = host(results["flags"]).astype(np.int64)
    rows, cols = host(rows).astype(np.int64), host(cols).astype(np.int64)
    poses = np.asarray(host(poses), dtype=np.float64).reshape(-1, 12)
    ok = ((flags & (1 | 2 | 8)) == 0) & (rows >= 0) & (cols >= 0)
    r, c = np.where(ok, rows, 0), np.where(ok, cols, 0)
    head = np.arctan2(poses[:, 2], poses[:, 0])
    dx, dz = poses[r, 3] - poses[c, 3], poses[r, 11] - poses[c, 11]
    cb, sb = np.cos(head[c]), np.sin(head[c])
    tx, ty = cb * dx + sb * dz, -sb * dx + cb * dz
    yaw = np.arctan2(ref[..., 1], ref[..., 0])
    dyaw = yaw - (head[r] - head[c])
    dyaw = np.abs((dyaw + np.pi) % (2.0 * np.pi) - np.pi)
    yaw_deg = np.where(ok, np.degrees(dyaw), np.nan)
    trans = np.where(ok, np.hypot(ref[..., 2] - tx, ref[..., 3] - ty), np.nan)
    some = bool(np.isfinite(yaw_deg).any())
    return {"yaw_deg": yaw_deg, "trans_m": trans,
            "median_yaw_deg": float(np.nanmedian(yaw_deg)) if some else float("nan"),
            "median_trans_m": float(np.nanmedian(trans)) if some else float("nan")}


def trajectory_error(est, truth, starts=None):
    """RMS position error (m) of estimated planar poses against the truth after ONE rigid planar alignment (rotation +
    translation, closed form: the least-squares fit of the positions).  est, truth: [M, 4] planar poses (c, s, x, y) or
    [M, 2] positions.  starts = None -> a float for the whole map (a merged multi-session map is only right when its
    sessions share one frame); starts = a session table -> float64 [S], every session aligned on its own (NaN for an
    empty one)."""
    def xy(a):
        a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)
        a = a.reshape(-1, a.shape[-1])
        return a[:, -2] + 1j * a[:, -1]

    def one(a, b):
        if a.size == 0:
            return float("nan")
        a, b = a - a.mean(), b - b.mean()
        rot = np.vdot(a, b)
        rot = rot / abs(rot) if abs(rot) > 0 else 1.0
        return float(np.sqrt(np.mean(np.abs(rot * a - b) ** 2)))

    a, b = xy(est), xy(truth)
    if a.shape != b.shape:
        raise ValueError("trajectory_error: est and truth must hold the same number of poses")
    if starts is None:
        return one(a, b)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    ends = np.append(starts[1:], a.size)
    return np.array([one(a[s:e], b[s:e]) for s, e in zip(starts, ends)], dtype=np.float64)


def localization_errors(pose, truth):
    """Translation and yaw error of localised scans (localize.localize / SG.localize) against the true
    poses.  pose, truth: planar poses [Q, 4] (c, s, x, y) in one frame; a query without a pose holds NaN and gets NaN
    errors.  -> dict: trans_m, yaw_deg (float64 numpy [Q]; the yaw error is the absolute angle between the two headings),
    median_trans_m, median_yaw_deg (NaN-ignoring; NaN when no query has a pose)."""
    def host(t):
        return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64).reshape(-1, 4)
    p, t = host(pose), host(truth)
    if p.shape != t.shape:
        raise ValueError("localization_errors: pose and truth must hold the same number of poses")
    trans = np.hypot(p[:, 2] - t[:, 2], p[:, 3] - t[:, 3])
    yaw = np.degrees(np.abs(np.arctan2(p[:, 1] * t[:, 0] - p[:, 0] * t[:, 1], p[:, 0] * t[:, 0] + p[:, 1] * t[:, 1])))
    some = bool(np.isfinite(trans).any())
    return {"trans_m": trans, "yaw_deg": yaw, "median_trans_m": float(np.nanmedian(trans)) if some else float("nan"),
            "median_yaw_deg": float(np.nanmedian(yaw)) if some else float("nan")}


def map_sharpness(lm, min_count=2):
    """A map-quality number that needs no ground truth: how tightly the observations of the landmarks
    of landmarks.build / SG.landmark_map sit on them.  lm: its dict ("count", "spread", "sessions").
    -> dict: sharpness = sqrt(sum count spread^2 / sum count) over the landmarks with count >= min_count, in metres (NaN
    without one); landmarks = how many those are; shared = the share of them seen by at least 2 sessions; single = the
    share of ALL landmarks with one observation.  Drift smears the observations of an object (sharpness rises) until
    they no longer link and the object splits into one landmark per session (shared falls, the count rises)."""
    def host(t):
        return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t).reshape(-1)
    count = host(lm["count"]).astype(np.int64)
    spread = host(lm["spread"]).astype(np.float64)
    words = host(lm["sessions"]).astype(np.int64).view(np.uint64)
    seen_by = np.zeros(words.shape, dtype=np.int64)
    for b in range(64):
        seen_by += ((words >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    big = count >= int(min_count)
    n = int(big.sum())
    w = count[big].astype(np.float64)
    return {"sharpness": float(np.sqrt(np.sum(w * spread[big] ** 2) / np.sum(w))) if n else float("nan"),
            "landmarks": n,
            "shared": float(np.mean(seen_by[big] >= 2)) if n else float("nan"),
            "single": float(np.mean(count == 1)) if count.size else float("nan")}
