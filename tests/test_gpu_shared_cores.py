"""The counting core that sgpr_pair_threshold_counts and the fused sgpr_score_threshold_counts (and its row-block path)
share (sgpr_eval.hpp), and the row lists of sgpr_topk_rows / sgpr_mine_rows behind the shared K dispatch, pinned against
references that share nothing with the kernels: metrics.counts_of (numpy searchsorted / bincount) for the counts and
masked numpy / torch sorts for the lists.  The mutual-equality tests of test_gpu_eval_pooled / test_gpu_topk compare two
routes through the same device code; these do not.  Shapes are the smallest at which the paths can go wrong: odd and even
T (the slab's padding to an even word count), T at the power-of-two edge of the tree and at each route's maximum, one to
three rank groups per threshold, ties across lanes and within a lane, NaN, +inf, -inf, rows with fewer than k entries."""
import numpy as np
import pytest
import torch

from test_gpu_mine import D_NEG, D_POS
from test_gpu_row_blocks import M_A, RB_A, _assert_row_blocked, _rb
from test_gpu_score_range import _any_shape
from test_gpu_topk import _reference as _topk_reference

pytestmark = pytest.mark.gpu

R, M = 37, 131


@pytest.fixture(scope="module")
def eng(ckpt_path):
    from sg_pr_amd import engine
    from oracle import sgpr_oracle
    e = engine.Engine(sgpr_oracle.load_checkpoint(ckpt_path), device=0)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------- counts
def _unusable(s):
    return np.isnan(s) | (s < 0)


def _counter(s, gt):
    """want(thr, rank) -> (counts [T + 1], skipped, rank sum) of metrics.counts_of (which sorts the negatives once); a
    negative pair with a negative / NaN score is skipped"""
    from sg_pr_amd import metrics
    bad = (gt == 0) & _unusable(s)
    g = gt.copy()
    g[bad] = -1
    count_fn = metrics.counts_of(s, g)[1]
    return lambda thr, rank: (*count_fn(thr, rank), int(bad.sum()))


def _want_counts(s, gt, thr, rank):
    counts, rank_sum, skipped = _counter(s, gt)(thr, rank)
    return counts, skipped, rank_sum


def _rank(s, gt, step):
    """thresholds and the rank triple (values, step, above) of the usable positives, `step` values per threshold"""
    from sg_pr_amd import metrics
    u, mult = metrics.distinct_counts(s[(gt == 1) & ~_unusable(s)])
    above = np.concatenate((np.cumsum(mult[::-1])[::-1], [0])).astype(np.int64)
    return u[::step], (u, step, above)


def _thresholds(s, gt, t):
    """exactly t ascending distinct thresholds: distinct positive scores, padded with a linspace"""
    u = np.unique(s[(gt == 1) & ~_unusable(s)])
    base = u[::max(1, -(-u.size // max(t, 1)))][:t]
    pad = np.linspace(0.0005, 0.9995, max(t, 1)).astype(np.float32)
    pad = pad[~np.isin(pad, base)][:t - base.size]
    thr = np.unique(np.concatenate((base, pad))).astype(np.float32)
    assert thr.size == t
    return thr


@pytest.fixture(scope="module")
def rect(eng):
    """37 x 131 pooled rectangle (the last column a copy of column 5: equal scores), explicit labels with ignored cells.
    -> rows, cols, the scores (numpy), gt, and the matrix route's scores with NaN / negative / infinite entries"""
    g = torch.Generator().manual_seed(11)
    rows, cols = (torch.randn(R, 32, generator=g) * 3.0).cuda(), (torch.randn(M, 32, generator=g) * 3.0).cuda()
    cols[M - 1] = cols[5]
    s = eng.score_all_pairs(rows, cols).cpu().numpy()
    gt = np.random.default_rng(7).choice(np.array([-1, 0, 1], dtype=np.int8), size=(R, M), p=[0.1, 0.6, 0.3])
    r_min = int(np.argmin(s)) // M
    r_eq, r_bad = (r_min + 1) % R, (r_min + 2) % R
    gt[s == s.min()] = 0                                  # a negative below every positive: bucket 0
    assert s[r_eq, 5].view(np.uint32) == s[r_eq, M - 1].view(np.uint32)
    gt[r_eq, 5], gt[r_eq, M - 1] = 1, 0                   # a negative equal to a positive value: the eq term
    assert s[gt == 1].min() > s.min()
    s2 = s.copy()
    s2[r_bad, :5] = [np.nan, -0.25, np.nan, -np.inf, np.inf]
    gt[r_bad, :5] = [0, 0, 1, 0, 0]
    return rows, cols, s, gt, s2


def _check_counts(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "counts")
    assert got[1] == want[1], (what, "skipped", got[1], want[1])
    assert got[2] == want[2], (what, "rank sum", got[2], want[2])


@pytest.mark.parametrize("t", [0, 1, 2, 3, 2047, 2048, 8191])
def test_matrix_counts(eng, rect, t):
    _, _, _, gt, s2 = rect
    thr = _thresholds(s2, gt, t)
    got = eng.pair_threshold_counts(torch.from_numpy(s2).cuda(), thr, gt=torch.from_numpy(gt).cuda())
    want = _want_counts(s2, gt, thr, None)
    assert want[1] == 3 and int(want[0].sum()) == int((gt == 0).sum()) - 3
    _check_counts(got, want, ("matrix", t))


@pytest.mark.parametrize("t", [0, 1, 2, 3, 2046, 2047])
def test_fused_counts(eng, rect, t):
    rows, cols, s, gt, _ = rect
    thr = _thresholds(s, gt, t)
    got = eng.score_threshold_counts(rows, cols, thr, gt=torch.from_numpy(gt).cuda())
    want = _want_counts(s, gt, thr, None)
    assert want[1] == 0 and int(want[0].sum()) == int((gt == 0).sum())
    _check_counts(got, want, ("fused", t))


@pytest.mark.parametrize("step", [5, 12, 20])
def test_ranked_counts_both_routes(eng, rect, step):
    """one, two and three rank groups of eight values per threshold"""
    rows, cols, s, gt, s2 = rect
    assert -(-step // 8) == {5: 1, 12: 2, 20: 3}[step]
    gt_d = torch.from_numpy(gt).cuda()
    thr, rank = _rank(s2, gt, step)
    assert 3 < thr.size < 2047
    want = _want_counts(s2, gt, thr, rank)
    assert want[1] == 3 and want[2] > 0
    _check_counts(eng.pair_threshold_counts(torch.from_numpy(s2).cuda(), thr, gt=gt_d, rank=rank), want, ("matrix", step))
    thr, rank = _rank(s, gt, step)
    want = _want_counts(s, gt, thr, rank)
    _check_counts(eng.score_threshold_counts(rows, cols, thr, gt=gt_d, rank=rank), want, ("fused", step))


def test_counts_across_row_blocks():
    """The handle without fused epilogues: the call scores row blocks and the blocks' counts add up on the device."""
    any_eng = _any_shape(_any_shape())
    try:
        assert any_eng.any_shape
        m, r = M_A, RB_A + 1
        rb = _rb(r, m)
        assert rb < r
        _assert_row_blocked(any_eng, r, m, rb)
        g = torch.Generator().manual_seed(21)
        rows, cols = torch.randn(r, 48, generator=g).cuda(), torch.randn(m, 48, generator=g).cuda()
        u = torch.rand(r, m, generator=g)
        gt_t = torch.where(u < 0.0005, 1, torch.where(u < 0.1, -1, 0)).to(torch.int8)
        del u
        gt = gt_t.numpy()
        s = any_eng.score_all_pairs(rows, cols).cpu().numpy()
        assert (gt[:rb] == 1).any() and (gt[rb:] == 0).any()
        want = _counter(s, gt)
        for step, t in ((12, None), (None, 2047)):
            thr, rank = _rank(s, gt, step) if step else (_thresholds(s, gt, t), None)
            assert thr.size <= 2047
            got = any_eng.score_threshold_counts(rows, cols, thr, gt=gt_t.cuda(), rank=rank)
            counts, rank_sum, skipped = want(thr, rank)
            _check_counts(got, (counts, skipped, rank_sum), ("row blocks", step, t))
    finally:
        any_eng.close()


# ---------------------------------------------------------------------------------------------------------- row lists
LIST_ROW0 = 60        # own frames 60 .. 65: a window of 10 straddles the lane boundary at column 64


@pytest.fixture(scope="module")
def lists():
    """6 x 200, uploaded: few distinct values (ties across lanes and, 64 columns apart, within a lane), NaN, +inf, -inf,
    a row of NaN only and a row with three finite entries.  Column poses: 0.5 m apart on a line."""
    rng = np.random.default_rng(5)
    s = rng.choice(np.linspace(0.05, 0.95, 12).astype(np.float32), size=(6, 200))
    s[0, [7, 71, 135, 3, 10]] = 0.99                      # the maximum: three times in lane 7, and in lanes 3 and 10
    s[1, rng.choice(200, 20, replace=False)] = np.nan
    s[1, [50, 114, 120]] = np.inf
    s[1, [0, 64, 128, 55, 62, 150]] = -np.inf
    s[2] = np.nan
    s[3] = -np.inf
    s[3, [1, 57, 130]] = [0.3, 0.7, 0.3]
    s[3, [2, 66, 140]] = np.nan
    s[4] = 0.5
    s[5, rng.choice(200, 40, replace=False)] = -np.inf
    s[5, [20, 84, 61]] = np.inf
    xz = np.stack((np.arange(200) * 0.5, np.zeros(200)), axis=1)
    return s, xz


@pytest.mark.parametrize("k", [1, 4, 8, 16])
@pytest.mark.parametrize("window", [-1, 0, 10])
def test_topk_rows_against_masked_sort(eng, lists, k, window):
    """admission on the value alone: a NaN or -inf entry is never listed, its slot stays (-inf, -1)"""
    s = torch.from_numpy(lists[0]).cuda()
    gv, gi = eng.topk_rows(s, k=k, row0=LIST_ROW0, window=window)
    wv, wi = _topk_reference(s, k, window, LIST_ROW0)
    assert torch.equal(gi, wi), (k, window, (gi != wi).nonzero()[:5].tolist())
    assert torch.equal(gv.view(torch.int32), wv.view(torch.int32)), (k, window)
    finite = sum(abs(c - (LIST_ROW0 + 3)) > window for c in (1, 57, 130))      # row 3: fewer than k for k > 3
    assert (gi[2] == -1).all() and int((gi[3] >= 0).sum()) == min(k, finite)


def _mine_want(s, xz, k, positives, window, causal):
    """masked sort with the float64 class rule of test_gpu_mine's reference; order: value (descending, or ascending for
    the positives), then column; an eligible -inf / +inf score is listed with its column"""
    r, m = s.shape
    self_ = np.arange(r, dtype=np.int64) + LIST_ROW0
    d = np.sqrt(((xz[self_][:, None, :] - xz[None, :, :]) ** 2).sum(2))
    c = np.arange(m)[None, :]
    dc = c - self_[:, None]
    good = ((d <= D_POS) if positives else (d >= D_NEG)) & ~np.isnan(s) & (dc != 0)
    if window >= 0:
        good &= np.abs(dc) > window
    if causal:
        good &= c < self_[:, None] - max(window, 0)
    vals = np.full((r, k), np.inf if positives else -np.inf, dtype=np.float32)
    idx = np.full((r, k), -1, dtype=np.int32)
    for i in range(r):
        cols = np.flatnonzero(good[i])
        key = s[i, cols].astype(np.float64) * (1.0 if positives else -1.0)
        order = cols[np.lexsort((cols, key))][:k]
        vals[i, :order.size] = s[i, order]
        idx[i, :order.size] = order
    return vals, idx


@pytest.mark.parametrize("k", [1, 4, 8, 16])
@pytest.mark.parametrize("positives", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_mine_rows_against_masked_sort(eng, lists, k, positives, causal):
    """admission by the total order (value, column): NaN never qualifies, an eligible -inf score does"""
    s, xz = lists
    assert (D_POS, D_NEG) == (3.0, 20.0)
    gv, gi = eng.mine_rows(torch.from_numpy(s).cuda(), xz, k=k, positives=positives, window=2, row0=LIST_ROW0,
                           causal=causal)
    wv, wi = _mine_want(s, xz, k, positives, 2, causal)
    gv, gi = gv.cpu().numpy(), gi.cpu().numpy()
    assert np.array_equal(gi, wi), (k, positives, causal, np.argwhere(gi != wi)[:5].tolist())
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), (k, positives, causal)
    assert (gi[2] == -1).all()
    if not positives and k > 1:                           # row 3: -inf scores listed with their columns
        assert np.isneginf(gv[3][gi[3] >= 0]).any()
