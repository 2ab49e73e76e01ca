"""sgpr_score_mine / sgpr_mine_rows: the hardest pose-labelled pairs per row without the similarity matrix - every index
and every value's bits against a stable sort of the dense matrix, masked in numpy with PairSet._targets' float64 rule."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D_POS, D_NEG = 3.0, 20.0


@pytest.fixture(scope="module")
def eng(ckpt_path):
    from sg_pr_amd import engine
    from oracle import sgpr_oracle
    e = engine.Engine(sgpr_oracle.load_checkpoint(ckpt_path), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(eng):
    """A KITTI-00-sized sequence of one world (revisits in its last third): pooled vectors and planar poses."""
    from sg_pr_amd import synth
    centers, labels, _, poses = synth.world_sequence(4541, 100, seed=7)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    return pooled, np.ascontiguousarray(poses[:, [3, 11]], dtype=np.float64)


def _reference(score, col_xz, k, positives, d_pos=D_POS, d_neg=D_NEG, window=-1, row0=0, causal=False, row_self=None,
               row_xz=None):
    """(values f32 [R,k], indices i32 [R,k]) from the dense matrix: mask, then a stable sort."""
    score = np.asarray(score, dtype=np.float32)
    r, m = score.shape
    self_ = np.arange(r, dtype=np.int64) + row0 if row_self is None else np.asarray(row_self, dtype=np.int64)
    if row_xz is None:
        ok = (self_ >= 0) & (self_ < m)
        row_xz = np.full((r, 2), np.nan)
        row_xz[ok] = col_xz[self_[ok]]
    # PairSet._targets' arithmetic: np.sqrt(((a - b) ** 2).sum(1)), float64
    d = np.sqrt(((row_xz[:, None, :] - col_xz[None, :, :]) ** 2).sum(2))
    cls = (d <= d_pos) if positives else (d >= d_neg)
    c = np.arange(m)[None, :]
    dc = c - self_[:, None]
    good = cls & ~np.isnan(score) & (dc != 0)
    if window >= 0:
        good &= np.abs(dc) > window
    if causal:
        good &= c < self_[:, None] - max(window, 0)
    key = np.where(good, score if positives else -score, np.inf).astype(np.float64)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    taken = np.take_along_axis(good, order, axis=1)
    vals = np.where(taken, np.take_along_axis(score, order, axis=1), np.float32(np.inf if positives else -np.inf))
    idx = np.where(taken, order, -1).astype(np.int32)
    if idx.shape[1] < k:
        pad = k - idx.shape[1]
        vals = np.concatenate((vals, np.full((r, pad), np.inf if positives else -np.inf, np.float32)), axis=1)
        idx = np.concatenate((idx, np.full((r, pad), -1, np.int32)), axis=1)
    return vals.astype(np.float32), idx


def _same(got, want, what):
    gv, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    wv, wi = want
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5])
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), what


@pytest.mark.parametrize("k", [1, 4, 8, 16])
@pytest.mark.parametrize("positives", [False, True])
def test_fused_equals_masked_sort(eng, world, k, positives):
    pooled, xz = world
    rows, cols = pooled[2900:3400].contiguous(), pooled[:3600].contiguous()
    cxz = xz[:3600]
    score = eng.score_all_pairs(rows, cols).cpu().numpy()
    for window, causal in ((-1, False), (50, False), (50, True), (-1, True)):
        got = eng.score_mine(rows, cols, cxz, k=k, positives=positives, window=window, row0=2900, causal=causal)
        want = _reference(score, cxz, k, positives, window=window, row0=2900, causal=causal)
        _same(got, want, ("row0", k, positives, window, causal))
    # row_self (a permutation with repeats) and separate row poses
    rs = np.random.default_rng(k).integers(0, 3600, size=500).astype(np.int32)
    got = eng.score_mine(rows, cols, cxz, k=k, positives=positives, window=50, row_self=torch.from_numpy(rs))
    _same(got, _reference(score, cxz, k, positives, window=50, row_self=rs), ("row_self", k, positives))
    rxz = xz[2900:3400] + np.random.default_rng(1).normal(0.0, 2.0, size=(500, 2))
    got = eng.score_mine(rows, cols, cxz, k=k, positives=positives, window=50, row0=2900, row_pose=rxz)
    _same(got, _reference(score, cxz, k, positives, window=50, row0=2900, row_xz=rxz), ("row_pose", k, positives))
    # mine_rows: the same lists from the resident matrix
    mr = eng.mine_rows(torch.from_numpy(score).cuda(), cxz, k=k, positives=positives, window=50, row0=2900, causal=True)
    fu = eng.score_mine(rows, cols, cxz, k=k, positives=positives, window=50, row0=2900, causal=True)
    assert torch.equal(mr[1], fu[1]) and torch.equal(mr[0].view(torch.int32), fu[0].view(torch.int32))


@pytest.mark.parametrize("k", [1, 16])
def test_full_kitti00_sized_sequence(eng, world, k):
    pooled, xz = world
    score = eng.score_all_pairs(pooled, pooled).cpu().numpy()
    for positives in (False, True):
        got = eng.score_mine(pooled, pooled, xz, k=k, positives=positives, window=50)
        _same(got, _reference(score, xz, k, positives, window=50), ("kitti00", k, positives))
        if positives:
            assert (got[1][:, 0] >= 0).sum().item() > 500            # the revisits are found
        again = eng.score_mine(pooled, pooled, xz, k=k, positives=positives, window=50)
        assert torch.equal(got[1], again[1]) and torch.equal(got[0].view(torch.int32), again[0].view(torch.int32))


def test_class_boundaries_nan_and_short_rows(eng, world):
    """Poses at exactly d_pos / d_neg and one float64 ulp either side (along x, z and a diagonal), NaN poses, NaN scores
    and rows with fewer than k eligible columns."""
    pooled, _ = world
    m = 600
    cols = pooled[:m].clone()
    cols[7] = float("nan")                                                # NaN inputs: the matrix path is the reference
    rng = np.random.default_rng(3)
    cxz = rng.uniform(-40.0, 40.0, size=(m, 2))
    edge = []
    for d in (D_POS, D_NEG):
        for v in (np.nextafter(d, 0.0), d, np.nextafter(d, np.inf)):
            edge += [(v, 0.0), (0.0, v), (-v, 0.0), (v * 0.6, v * 0.8)]
    cxz[100:100 + len(edge)] = np.array(edge)
    cxz[300] = (np.nan, 0.0)
    cxz[301] = (0.0, np.nan)
    r = 40
    rows = pooled[1000:1000 + r].contiguous()
    rxz = np.zeros((r, 2))
    rxz[5] = (np.nan, np.nan)                                             # a row that gets nothing
    rxz[6:10] = rng.uniform(-1.0, 1.0, size=(4, 2))
    rows[11] = float("nan")
    score = eng.score_all_pairs(rows, cols).cpu().numpy()
    # the NaN graphs really are NaN in the matrix (not scored like a healthy graph upstream)
    assert np.isnan(score[11]).all() and np.isnan(score[:, 7]).all()
    for k in (1, 4, 16):
        for positives in (False, True):
            got = eng.score_mine(rows, cols, cxz, k=k, positives=positives, row_self=torch.arange(r, dtype=torch.int32) + 120,
                                 row_pose=rxz)
            assert (got[1][11] == -1).all() and (got[1] != 7).all()    # ... and absent from the lists
            want = _reference(score, cxz, k, positives, row_self=np.arange(r) + 120, row_xz=rxz)
            _same(got, want, ("edges", k, positives))
            assert (got[1][5] == -1).all()                             # the NaN row pose: nothing qualifies
            assert not torch.isnan(got[0]).any()                           # a NaN score is never reported
    # short rows: 10 columns, k = 16
    got = eng.score_mine(rows, cols[:10], cxz[:10], k=16, positives=False, row_pose=rxz)
    want = _reference(score[:, :10], cxz[:10], 16, False, row_xz=rxz)
    _same(got, want, "short")
    assert (got[1][:, 10:] == -1).all()


def test_fallback_handles(eng, world):
    """The wide-range instance (debug bit 13) and an any-shape handle score row blocks and run sgpr_mine_rows' kernel:
    bit-equal to mine_rows on their own matrix."""
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    pooled, xz = world
    rows, cols = pooled[3000:3300].contiguous(), pooled[:1800].contiguous()
    eng.set_skip_mask(1 << 13)
    try:
        score = eng.score_all_pairs(rows, cols)
        for k, positives, causal in ((1, False, False), (4, True, True), (16, True, False), (16, False, True)):
            got = eng.score_mine(rows, cols, xz[:1800], k=k, positives=positives, window=10, row0=3000, causal=causal,
                                 row_pose=xz[3000:3300])
            want = eng.mine_rows(score, xz[:1800], k=k, positives=positives, window=10, row0=3000, causal=causal,
                                 row_pose=xz[3000:3300])
            assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
            _same(got, _reference(score.cpu().numpy(), xz[:1800], k, positives, window=10, row0=3000, causal=causal,
                                  row_xz=xz[3000:3300]), ("wide", k, positives))
    finally:
        eng.set_skip_mask(0)
    args = sgpr_args()
    args.filters_1, args.filters_2, args.filters_3, args.tensor_neurons, args.bottle_neck_neurons = 64, 64, 48, 16, 16
    args.node_num, args.K = 64, 10
    torch.manual_seed(5)
    model = sg_net.SG(args, 12).eval()
    e2 = model.engine()
    assert e2.any_shape
    g = torch.Generator().manual_seed(6)
    pr, pc = torch.randn(33, 48, generator=g).cuda(), torch.randn(150, 48, generator=g).cuda()
    pxz = np.cumsum(np.random.default_rng(2).normal(0.0, 2.0, size=(150, 2)), axis=0)
    score = e2.score_all_pairs(pr, pc)
    for k, positives in ((1, False), (3, True), (16, False)):
        got = model.hard_pairs(pr, pc, pxz, k=k, positives=positives, window=2)
        want = e2.mine_rows(score, pxz, k=k, positives=positives, window=2)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        _same(got, _reference(score.cpu().numpy(), pxz, k, positives, window=2), ("any-shape", k, positives))


def test_workspace_far_below_the_matrix(eng):
    n = 100000
    for k in (1, 16):
        for positives in (False, True):
            ws = eng.score_mine_workspace_bytes(n, n, k, positives=positives)
            assert 0 < ws < 0.01 * 4 * n * n, ws


def test_row_self_out_of_range_is_reported(eng, world):
    from sg_pr_amd.engine import SgprError
    pooled, xz = world
    eng.score_mine(pooled[:4], pooled[:50], xz[:50], k=4, row_self=torch.tensor([0, 3, 50, 1], dtype=torch.int32))
    with pytest.raises(SgprError, match="row_self"):
        eng.check_status()
    eng.check_status()


def test_invalid_arguments(eng, world):
    pooled, xz = world
    lib = eng.lib
    rows, cols = pooled[:8].contiguous(), pooled[:64].contiguous()
    cp = torch.from_numpy(xz[:64].copy()).cuda()
    vals = torch.empty(8, 16, device="cuda")
    idx = torch.empty(8, 16, dtype=torch.int32, device="cuda")
    score = eng.score_all_pairs(rows, cols)
    need = lib.sgpr_score_mine_workspace_bytes(eng._h, 8, 64, 4, 2)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731

    def fused(h=eng._h, r=P(rows), c=P(cols), pose=P(cp), flags=2, dp=D_POS, dn=D_NEG, k=4, v=P(vals), i=P(idx),
              w=P(ws), wb=need, n=8, row0=0):
        return lib.sgpr_score_mine(h, r, n, c, 64, pose, None, None, row0, -1, flags, dp, dn, k, v, i, w, wb, None)

    def rows_(h=eng._h, pose=P(cp), flags=2, dp=D_POS, dn=D_NEG, k=4, v=P(vals), i=P(idx), s=P(score)):
        return lib.sgpr_mine_rows(h, s, 8, 64, 64, pose, None, None, 0, -1, flags, dp, dn, k, v, i, None, 0, None)

    for call in (fused, rows_):
        assert call() == 0
        assert call(h=None) == -1
        assert call(pose=None) == -1
        assert call(v=None) == -1 and call(i=None) == -1
        for k in (0, 17):
            assert call(k=k) == -1
        for flags in (0, 6, 1, 8 | 2, -1):
            assert call(flags=flags) == -1, flags
        assert call(dp=float("nan")) == -1 and call(dn=float("nan")) == -1
        assert call(dp=21.0) == -1
    assert fused(r=None) == -1 and fused(c=None) == -1
    assert fused(row0=0x7fffffff - 4) == -1
    assert rows_(s=None) == -1
    assert fused(wb=need - 1) == -7 and fused(w=None) == -7
    torch.cuda.synchronize()
    eng.check_status()
