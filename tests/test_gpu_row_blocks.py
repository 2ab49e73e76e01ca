"""The fused epilogues (score_topk, _mine, _above, _positives, _threshold_counts) on calls that run in more than one row
block, against the same handle's score_all_pairs on the SAME rectangle and the matrix kernels on it.

Where a call splits its rectangle (include/sgpr.h):
  wide-range (debug bit 13, out-of-range weights) and any-shape handles: score blocks of at most 64 MB (score_row_blocks)
  production handle, score_above / _positives / _threshold_counts: launches of at most 131 072 rows (AB_ROWS)
  any-shape plain-fp32 scorer: grid chunks of at most 65 535 rows
Every case asserts that it runs more than one block.  The references are score_all_pairs of the whole rectangle, the
matrix kernels (topk_rows, mine_rows, rows_above, pair_positives, pair_threshold_counts) and the masked stable sorts of
test_gpu_topk / test_gpu_mine / test_gpu_score_above; score_all_pairs itself is held to the float64 tail of
tests/score_ref.py on the rows at both sides of every block boundary, so that "equal to a wrong matrix" cannot pass.

The f16-range question (exact fp32, f16 planes, or f16 with the clamp-ReLU) belongs to the whole rectangle: one row far
outside the range, in the first or the last block, must put every block on the datapath score_all_pairs takes."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import score_ref
from test_gpu_eval_pooled import _counts_equal, _positives_equal, _rank_of
from test_gpu_mine import _reference as _mine_reference
from test_gpu_score_above import _equal as _above_equal
from test_gpu_score_above import _quantile
from test_gpu_score_above import _reference as _above_reference
from test_gpu_score_range import BAR, _any_shape, _tolerance, _wide_checkpoint
from test_gpu_stateless import _check_all_patterns, _trim
from test_gpu_topk import _reference as _topk_reference

pytestmark = pytest.mark.gpu

BLOCK_BYTES = 64 << 20      # score_row_blocks' block
AB_ROWS = 131072            # the production handle's longest launch (sgpr_score.hip)
GRID_Y = 65535              # the any-shape plain-fp32 scorer's grid chunk (sgpr_generic.hip)
D_POS, D_NEG = 3.0, 20.0


def _rb(r, m):
    return max(1, min(r, BLOCK_BYTES // (4 * m)))


# (M, R) of the 64 MB path: a last block of one row, blocks that divide evenly, ~3.4 blocks, many thin blocks
M_A = 4541
RB_A = _rb(1 << 30, M_A)
SHAPES = [(M_A, RB_A + 1), (M_A, 2 * RB_A), (M_A, int(3.4 * RB_A)), (262144, 150)]


# ---------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def sd(ckpt_path):
    from oracle import sgpr_oracle
    return sgpr_oracle.load_checkpoint(ckpt_path)


@pytest.fixture(scope="module")
def eng(sd):
    from sg_pr_amd import engine
    e = engine.Engine(sd, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wide_eng(sd):
    from sg_pr_amd import engine
    e = engine.Engine(_wide_checkpoint(sd), device=0)
    assert not e.uses_f16_planes()
    yield e
    e.close()


@pytest.fixture(scope="module")
def any_sd():
    return _any_shape()


@pytest.fixture(scope="module")
def any_eng(any_sd):
    e = _any_shape(any_sd)
    assert e.any_shape
    yield e
    e.close()


@pytest.fixture(scope="module")
def walk():
    """The first 1000 frames of the KITTI-like planar walk (1 m per frame): float64 [1000, 2]."""
    from sg_pr_amd import allpairs, synth
    return allpairs.pose_xz(synth.kitti_like_sequence(4541, 64, seed=3)[3]).numpy()[:1000]


def _poses(walk, n):
    """pose of frame i = walk[i mod 1000]: every block of rows revisits the places of the first 300 columns"""
    return np.ascontiguousarray(walk[np.arange(n) % walk.shape[0]])


def _pooled(n, width, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, width, generator=g) * scale).cuda()


def _handles(eng, wide_eng, any_eng, sd, any_sd):
    """(name, engine, debug mask, state dict of its tail, pooled width, input scale)"""
    return {"tuned, bit 13": (eng, 1 << 13, sd, 32, 3.0), "wide checkpoint": (wide_eng, 0, sd, 32, 3.0),
            "any-shape": (any_eng, 0, any_sd, 48, 1.0), "any-shape, bit 23": (any_eng, 1 << 23, any_sd, 48, 1.0)}


HANDLE_NAMES = ["tuned, bit 13", "wide checkpoint", "any-shape", "any-shape, bit 23"]


# ---------------------------------------------------------------------------------------------------------- checks
def _boundaries(r, rb):
    return list(range(rb, r, rb))


def _sample_rows(r, rb, extra=()):
    """32 rows on each side of every block boundary, the first and last row and any scaled row"""
    s = {0, r - 1, *extra}
    for b in _boundaries(r, rb):
        s.update(range(max(0, b - 32), min(r, b + 32)))
    return np.array(sorted(s), dtype=np.int64)


def _check_tail(e_sd, rows, cols, score, pick, cond=False, what=""):
    """score_all_pairs' rows `pick` within the float64 tail's bar (columns thinned to keep the reference small)"""
    m = cols.shape[0]
    cpick = np.arange(m) if m <= 8192 else np.unique(np.concatenate((np.arange(64), np.arange(m - 64, m),
                                                                      np.arange(0, m, 97))))
    cn = cols.cpu().numpy()[cpick]
    step = max(1, 1500000 // (cpick.size * 32))
    for a in range(0, pick.size, step):
        pr = pick[a:a + step]
        ref = score_ref.tail(e_sd, rows[torch.from_numpy(pr).cuda()].cpu().numpy(), cn)
        got = score[torch.from_numpy(pr).cuda()][:, torch.from_numpy(cpick).cuda()].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), (what, "not finite")
        d = np.abs(got - ref["score"])
        tol = _tolerance(ref, BAR, cond)
        assert (d <= tol).all(), (what, "score_all_pairs vs float64", float(d.max()), float((d - tol).max()))


def _classes_per_block(rxz, cxz, r, rb):
    """positives (<= D_POS) and negatives (>= D_NEG) in every block of rows: both classes must be populated"""
    rx, cx = torch.from_numpy(rxz).cuda(), torch.from_numpy(cxz).cuda()
    for b0 in range(0, r, rb):
        npos = nneg = 0
        for a in range(b0, min(r, b0 + rb), 2048):
            d = torch.cdist(rx[a:min(a + 2048, b0 + rb, r)], cx)
            npos += int((d <= D_POS).sum())
            nneg += int((d >= D_NEG).sum())
        assert npos > 0 and nneg > 0, ("a block without both classes", b0, npos, nneg)


def _assert_row_blocked(e, r, m, rb):
    """every epilogue's workspace holds one score block of rb rows, never the matrix: past rb rows it grows by O(R) bytes
    only (row pointers, counts), and once there are two full blocks it is below the matrix itself"""
    sizes = (lambda n: e.score_topk_workspace_bytes(n, m, 16), lambda n: e.score_mine_workspace_bytes(n, m, 16),
             lambda n: e.score_above_workspace_bytes(n, m), lambda n: e.score_positives_workspace_bytes(n, m),
             lambda n: e.score_threshold_counts_workspace_bytes(n, m, 2047))
    for ws in sizes:
        assert 0 < ws(rb) <= ws(r) <= ws(rb) + 16 * (r - rb) + 4096, (r, m, ws(rb), ws(r))
        assert r < 2 * rb or ws(r) < 4 * r * m, (r, m, ws(r))


def _topk_equal(got, want, what):
    gv, gi = got
    wv, wi = want
    bad = ((gv != wv) & ~(torch.isinf(gv) & torch.isinf(wv))) | (gi != wi)
    assert not bad.any(), (what, bad.nonzero()[:5].tolist())
    assert torch.equal(gv.view(torch.int32)[~torch.isinf(gv)], wv.view(torch.int32)[~torch.isinf(wv)]), what


def _mine_equal(got, want, what):
    assert torch.equal(got[1], want[1]), (what, "indices", (got[1] != want[1]).nonzero()[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (what, "values")


def _mine_vs_numpy(got, score, cxz, k, positives, pick, window=-1, row0=0, causal=False, row_self=None, row_xz=None,
                   what=""):
    """the numpy masked stable sort of test_gpu_mine on the rows `pick`, in row chunks (float64 distances [n, M, 2])"""
    m = score.shape[1]
    step = max(1, 2000000 // m)
    gv, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    for a in range(0, pick.size, step):
        pr = pick[a:a + step]
        sc = score[torch.from_numpy(pr).cuda()].cpu().numpy()
        rs = (np.asarray(row_self)[pr] if row_self is not None else (pr + row0)).astype(np.int64)
        wv, wi = _mine_reference(sc, cxz, k, positives, window=window, causal=causal, row_self=rs,
                                 row_xz=None if row_xz is None else row_xz[pr])
        assert np.array_equal(gi[pr], wi), (what, "mine indices vs numpy")
        assert np.array_equal(gv[pr].view(np.uint32), wv.view(np.uint32)), (what, "mine values vs numpy")


def _sub_multiset(part, whole):
    a, b = collections.Counter(part.tolist()), collections.Counter(whole.tolist())
    return all(b[v] >= c for v, c in a.items())


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _above_no_row_ptr(e, rows, cols, thr, window, want):
    """the raw C-ABI with d_row_ptr NULL: the row pointers live in the workspace (the row-block head's own)"""
    r, m = rows.shape[0], cols.shape[0]
    n = want[0].numel()
    out = [torch.empty(max(n, 1), dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32)]
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws_bytes = e.score_above_workspace_bytes(r, m)
    ws = e._ws(ws_bytes)
    rc = e.lib.sgpr_score_above(e._h, _vp(rows), r, _vp(cols), m, None, 0, window, 0, float(thr), _vp(out[0]),
                                _vp(out[1]), _vp(out[2]), n, None, _vp(count), _vp(ws), ws_bytes, _stream())
    e._check(rc)
    assert int(count) == n
    for g, w in zip(out, want[:3]):
        assert torch.equal(g[:n], w)


def _epilogues(e, e_sd, rows, cols, xz, rb, what):
    """All five epilogues on rows x cols against the whole rectangle's matrix; returns the matrix."""
    r, m = rows.shape[0], cols.shape[0]
    score = e.score_all_pairs(rows, cols)
    pick = _sample_rows(r, rb)
    _check_tail(e_sd, rows, cols, score, pick, what=what)
    row0 = 17
    cxz = xz[:m]
    rxz = xz[row0:row0 + r]
    # ---- top-k
    rs = torch.from_numpy(np.random.default_rng(r + m).integers(0, m, size=r).astype(np.int32))
    for k, window, r0, causal, rself in ((1, -1, 0, False, None), (16, 5, row0, True, None), (16, 3, 0, False, rs)):
        got = e.score_topk(rows, cols, k=k, window=window, row0=r0, causal=causal, row_self=rself)
        _topk_equal(got, _topk_reference(score, k, window, r0, causal, rself), (what, "score_topk", k, window, r0, causal))
    v, i = e.topk_rows(score, k=4, row0=row0, window=7)
    got = e.score_topk(rows, cols, k=4, window=7, row0=row0)
    assert torch.equal(got[1], i) and torch.equal(got[0].view(torch.int32), v.view(torch.int32)), (what, "topk_rows")
    # ---- mining: both modes, row poses given and omitted, row_self, causal
    noisy = rxz + np.random.default_rng(1).normal(0.0, 1.0, size=rxz.shape)
    for k, pos, causal, rpose, rself in ((16, False, False, None, None), (4, True, True, noisy, None),
                                         (1, True, False, None, rs), (16, False, True, noisy, rs)):
        kw = dict(k=k, positives=pos, window=5, row0=row0, causal=causal, row_pose=rpose,
                  row_self=None if rself is None else rself)
        got = e.score_mine(rows, cols, cxz, **kw)
        _mine_equal(got, e.mine_rows(score, cxz, **kw), (what, "score_mine", k, pos, causal))
        _mine_vs_numpy(got, score, cxz, k, pos, pick, window=5, row0=row0, causal=causal,
                       row_self=None if rself is None else rself.numpy(), row_xz=rpose, what=(what, k, pos, causal))
    # ---- range selection: unlimited, a capacity ending inside the second block, count only, no row pointer
    thr = _quantile(score[:min(r, 512)], 0.99)
    for causal in (False, True):
        want = _above_reference(score, thr, 5, row0, causal)
        _above_equal(e.score_above(rows, cols, thr, window=5, row0=row0, causal=causal), want, (what, "above", causal))
        cap = int(want[3][rb]) + 3                               # (inside the second block)
        assert causal or cap < int(want[3][-1])
        got = e.score_above(rows, cols, thr, window=5, row0=row0, causal=causal, capacity=cap)
        assert torch.equal(got[3], want[3]), (what, "above capacity: row_ptr")
        kk = min(cap, want[0].numel())
        for g, w in zip(got[:3], want[:3]):
            assert torch.equal(g[:kk], w[:kk]), (what, "above capacity")
        got = e.score_above(rows, cols, thr, window=5, row0=row0, causal=causal, capacity=0)
        assert torch.equal(got[3], want[3]), (what, "above count only")
    want = _above_reference(score, thr, 2, 0, False)
    _above_no_row_ptr(e, rows, cols, thr, 2, want)
    # ---- evaluation: pose truth with row0, gt truth, rankings of ~2047 and 7 thresholds
    xz_d = torch.from_numpy(xz).cuda()
    _, pos = _positives_equal(e, rows, cols, row0=row0, xz=xz_d, what=(what, "positives, poses"))
    for t in (2047, 7):
        thr_t, rank = _rank_of(pos, t)
        assert t // 2 < thr_t.size <= t                     # (_rank_of: every ceil(u / t)-th distinct value)
        _counts_equal(e, rows, cols, score, thr_t, row0=row0, xz=xz_d, rank=rank, what=(what, "counts", t))
    d = torch.cdist(torch.from_numpy(rxz).cuda(), torch.from_numpy(cxz).cuda())
    gt = torch.where(d <= D_POS, 1, torch.where(d >= D_NEG, 0, -1)).to(torch.int8)
    del d
    _, pos = _positives_equal(e, rows, cols, gt=gt, what=(what, "positives, gt"))
    thr_t, rank = _rank_of(pos, 7)
    _counts_equal(e, rows, cols, score, thr_t, gt=gt, rank=rank, what=(what, "counts, gt"))
    return score


# ---------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("shape", SHAPES, ids=["rb+1", "2rb", "3.4rb", "thin"])
@pytest.mark.parametrize("hname", HANDLE_NAMES)
def test_offsets_across_blocks(eng, wide_eng, any_eng, sd, any_sd, walk, hname, shape):
    """Uniform inputs on the fallback handles: every offset a block passes (row0 + r0, row_self + r0, row poses + 2 r0,
    outputs + r0 k, row pointers + r0, gt + r0 ldg) and every head region reused between blocks."""
    e, mask, e_sd, width, scale = _handles(eng, wide_eng, any_eng, sd, any_sd)[hname]
    m, r = shape
    rb = _rb(r, m)
    assert r > rb
    xz = _poses(walk, max(m, r + 17))
    _classes_per_block(xz[17:17 + r], xz[:m], r, rb)
    rows, cols = _pooled(r, width, scale, 3 + r), _pooled(m, width, scale, 4 + m)
    e.set_skip_mask(mask)                                # (the workspace sizes depend on the mask too)
    try:
        _assert_row_blocked(e, r, m, rb)
        _epilogues(e, e_sd, rows, cols, xz, rb, (hname, m, r))
    finally:
        e.set_skip_mask(0)


# ---------------------------------------------------------------------------------------------------------- (b)
def _scale_row(e_sd, row, cols, quantity, target, k):
    """the factor s at which one row (times s) against cols puts a range quantity of score_ref.gates at target"""
    def q(s):
        g = score_ref.gates(e_sd, row * np.float32(s), cols)
        return dict(bound=score_ref.bound(g, k), mode2=g["um"] + g["l1"] * g["em"])[quantity]
    lo, hi = 1e-3, 1e8
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        lo, hi = (mid, hi) if q(mid) < target else (lo, mid)
    return float(np.sqrt(lo * hi))


def _rows_quantity(e_sd, rows_np, cols_np, quantity, k):
    """max over rows of the range quantity, in row chunks"""
    best = 0.0
    for a in range(0, rows_np.shape[0], 8192):
        g = score_ref.gates(e_sd, rows_np[a:a + 8192], cols_np)
        best = max(best, dict(bound=score_ref.bound(g, k), mode2=g["um"] + g["l1"] * g["em"])[quantity])
    return best


def _mixed(e, e_sd, rows, cols, xz, rb, where, quantity, thr, k, what):
    """rows with row `where` scaled to 1.03x the gate; every epilogue against the whole rectangle's matrix"""
    from sg_pr_amd import metrics
    r, m = rows.shape[0], cols.shape[0]
    rn, cn = rows.cpu().numpy(), cols.cpu().numpy()
    assert _rows_quantity(e_sd, rn, cn, quantity, k) < 0.97 * thr            # the rest of the rows: inside the gate
    s = _scale_row(e_sd, rn[where:where + 1], cn, quantity, 1.03 * thr, k)
    rows = rows.clone()
    rows[where] *= s
    g = score_ref.gates(e_sd, rows[where:where + 1].cpu().numpy(), cn)
    got_q = dict(bound=score_ref.bound(g, k), mode2=g["um"] + g["l1"] * g["em"])[quantity]
    assert abs(got_q / (1.03 * thr) - 1.0) < 1e-3
    score = e.score_all_pairs(rows, cols)
    # non-vacuity: the block without the scaled row, scored alone, is on the other side of the gate
    b0 = 0 if where >= rb else rb * ((r - 1) // rb)
    alone = e.score_all_pairs(rows[b0:b0 + rb].contiguous(), cols)
    ndiff = int((alone.view(torch.int32) != score[b0:b0 + rb].view(torch.int32)).sum())
    if quantity == "bound":
        assert ndiff > 0, (what, "the block alone gives the same bits: the case cannot tell the behaviours apart")
    else:
        assert ndiff == 0, (what, "the clamp form of the f16 path changed bits", ndiff)   # sgpr_score.hip split_relu4
    pick = _sample_rows(r, rb, extra=(where,))
    _check_tail(e_sd, rows, cols, score, pick, cond=True, what=what)
    row0 = 5
    cxz = xz[:m]
    for kk, window, causal in ((1, -1, False), (16, 5, True)):
        got = e.score_topk(rows, cols, k=kk, window=window, row0=row0, causal=causal)
        _topk_equal(got, _topk_reference(score, kk, window, row0, causal), (what, "score_topk", kk))
    for pos in (False, True):
        kw = dict(k=8, positives=pos, window=5, row0=row0)
        _mine_equal(e.score_mine(rows, cols, cxz, **kw), e.mine_rows(score, cxz, **kw), (what, "score_mine", pos))
    thr_a = _quantile(score[:2048], 0.99)
    for causal in (False, True):
        want = _above_reference(score, thr_a, 5, row0, causal)
        _above_equal(e.score_above(rows, cols, thr_a, window=5, row0=row0, causal=causal), want, (what, "score_above"))
    xz_d = torch.from_numpy(xz).cuda()
    _, pos = _positives_equal(e, rows, cols, row0=row0, xz=xz_d, what=(what, "positives"))
    thr_t, rank = _rank_of(pos, 2047)
    _counts_equal(e, rows, cols, score, thr_t, row0=row0, xz=xz_d, rank=rank, what=(what, "counts"))
    assert metrics.pr_roc_pooled(e, rows, cols, pose_xz=xz_d, row0=row0)[:2] == \
        metrics.pr_roc_device(e, score, pose_xz=xz_d, row0=row0)[:2], (what, "pr_roc_pooled")
    return ndiff


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("gate", ["bound", "mode2"])
def test_mixed_range_production_handle(eng, sd, walk, gate, where):
    """R = 131072 + 37: score_above / _positives / _threshold_counts run two launches; one row beyond the exact-path gate
    (60000) or the clamp-form gate (1024) must decide the datapath of both.  score_topk / score_mine: one launch
    (controls)."""
    r, m = AB_ROWS + 37, 300
    xz = _poses(walk, r + 5)
    _classes_per_block(xz[5:5 + r], xz[:m], r, AB_ROWS)
    rows, cols = _pooled(r, 32, 1.0, 41), _pooled(m, 32, 1.0, 42)
    thr = score_ref.F16_SAFE if gate == "bound" else score_ref.MODE2_BOUND
    idx = 5 if where == "first" else r - 3
    _mixed(eng, sd, rows, cols, xz, AB_ROWS, idx, gate, thr, score_ref.TUNED_K, ("tuned", gate, where))


@pytest.mark.parametrize("where", ["first", "last"])
def test_mixed_range_any_shape_handle(any_eng, any_sd, walk, where):
    """The any-shape matrix-core tail on the 64 MB path (last block of one row): one row beyond its gate decides the
    whole rectangle."""
    m = M_A
    rb = RB_A
    r = rb + 1
    _assert_row_blocked(any_eng, r, m, rb)
    xz = _poses(walk, max(m, r + 5))
    rows, cols = _pooled(r, 48, 1.0, 43), _pooled(m, 48, 1.0, 44)
    idx = 3 if where == "first" else r - 1
    _mixed(any_eng, any_sd, rows, cols, xz, rb, idx, "bound", score_ref.F16_SAFE, score_ref.ANY_SHAPE_K,
           ("any-shape", where))


# ---------------------------------------------------------------------------------------------------------- (c)
def test_production_long_evaluation_calls(eng, sd, walk):
    """score_positives / score_threshold_counts with R = 131072 + 37 on uniform inputs: pose truth with row0, gt truth
    with ldg > M (labels offset per block), and a positives capacity that ends inside the second block."""
    r, m, row0, ldg = AB_ROWS + 37, 300, 9, 317
    xz = _poses(walk, r + row0)
    _classes_per_block(xz[row0:row0 + r], xz[:m], r, AB_ROWS)
    rows, cols = _pooled(r, 32, 3.0, 51), _pooled(m, 32, 3.0, 52)
    xz_d = torch.from_numpy(xz).cuda()
    score, pos = _positives_equal(eng, rows, cols, row0=row0, xz=xz_d, what="poses")
    _check_tail(sd, rows, cols, score, _sample_rows(r, AB_ROWS), what="long eval")
    for t in (2047, 5):
        thr, rank = _rank_of(pos, t)
        _counts_equal(eng, rows, cols, score, thr, row0=row0, xz=xz_d, rank=rank, what=("counts", t))
    # gt [R][ldg], ldg > M: the raw entry points (the binding passes ldg = M); the matrix path on gt[:, :M]
    d = torch.cdist(xz_d[row0:row0 + r], xz_d[:m])
    lab = torch.where(d <= D_POS, 1, torch.where(d >= D_NEG, 0, -1)).to(torch.int8)
    del d
    gt = torch.full((r, ldg), 1, dtype=torch.int8, device="cuda")   # (the padding would count as positives if read)
    gt[:, :m] = lab
    want, wbad = eng.pair_positives(score, gt=lab)
    lib, h = eng.lib, eng._h
    ws_bytes = lib.sgpr_score_positives_workspace_bytes(h, r, m)
    ws = eng._ws(ws_bytes)
    out = torch.empty(want.numel() + 16, dtype=torch.float32, device="cuda")
    cnt = torch.empty(2, dtype=torch.int64, device="cuda")
    assert lib.sgpr_score_positives(h, _vp(rows), r, _vp(cols), m, 0, None, 3.0, 20.0, _vp(gt), ldg, _vp(out), out.numel(),
                                    _vp(cnt), _vp(ws), ws_bytes, _stream()) == 0
    n, bad = (int(v) for v in cnt.tolist())
    assert (n, bad) == (want.numel(), wbad)
    assert torch.equal(torch.sort(out[:n].view(torch.int32))[0], torch.sort(want.view(torch.int32))[0])
    thr, rank = _rank_of(want, 64)
    wc = eng.pair_threshold_counts(score, thr, gt=lab)
    t = thr.size
    dthr = torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float32)).cuda()
    res = torch.empty(t + 3, dtype=torch.int64, device="cuda")
    nb = lib.sgpr_score_threshold_counts_workspace_bytes(h, r, m, t)
    ws = eng._ws(nb)
    assert lib.sgpr_score_threshold_counts(h, _vp(rows), r, _vp(cols), m, 0, None, 3.0, 20.0, _vp(gt), ldg, _vp(dthr), t,
                                           None, 0, None, _vp(res), _vp(ws), nb, _stream()) == 0
    hres = res.cpu().numpy()
    assert np.array_equal(hres[:t + 1], wc[0]) and int(hres[t + 1]) == wc[1]
    # a capacity that ends inside the second block: the count stays exact, the written prefix is a sub-multiset
    n1 = eng.pair_positives(score[:AB_ROWS], row0=row0, pose_xz=xz_d)[0].numel()
    assert 0 < n1 < pos.numel() - 3
    cap = n1 + 3
    out = torch.full((cap,), float("nan"), dtype=torch.float32, device="cuda")
    ws_bytes = lib.sgpr_score_positives_workspace_bytes(h, r, m)
    ws = eng._ws(ws_bytes)
    assert lib.sgpr_score_positives(h, _vp(rows), r, _vp(cols), m, row0, _vp(xz_d), 3.0, 20.0, None, m, _vp(out), cap,
                                    _vp(cnt), _vp(ws), ws_bytes, _stream()) == 0
    assert int(cnt[0]) == pos.numel()
    assert _sub_multiset(out.view(torch.int32).cpu().numpy(), pos.view(torch.int32).cpu().numpy())
    eng.check_status()


# ---------------------------------------------------------------------------------------------------------- (d)
def test_any_shape_scorer_past_65535_rows(any_eng, any_sd):
    """Bit 23 (plain fp32, no gate) with R = 65535 + 37: the second grid chunk's rows equal a separate call on them and
    the float64 tail; without bit 23 one scaled row sends both grid chunks through the same gate word."""
    r, m = GRID_Y + 37, 40
    rows, cols = _pooled(r, 48, 1.0, 61), _pooled(m, 48, 1.0, 62)
    any_eng.set_skip_mask(1 << 23)
    try:
        score = any_eng.score_all_pairs(rows, cols)
        tail = any_eng.score_all_pairs(rows[65500:].contiguous(), cols)
        assert torch.equal(score[65500:].view(torch.int32), tail.view(torch.int32))
        head = any_eng.score_all_pairs(rows[:100].contiguous(), cols)
        assert torch.equal(score[:100].view(torch.int32), head.view(torch.int32))
        pick = np.concatenate((np.arange(32), np.arange(GRID_Y - 32, r)))
        _check_tail(any_sd, rows, cols, score, pick, what="bit 23, 65572 rows")
        where = GRID_Y + 5
        s = _scale_row(any_sd, rows[where:where + 1].cpu().numpy(), cols.cpu().numpy(), "bound", 1.03 * score_ref.F16_SAFE,
                       score_ref.ANY_SHAPE_K)
        mixed = rows.clone()
        mixed[where] *= s
        plain = any_eng.score_all_pairs(mixed, cols)
    finally:
        any_eng.set_skip_mask(0)
    got = any_eng.score_all_pairs(mixed, cols)
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), "both grid chunks on the plain-fp32 path"
    alone = any_eng.score_all_pairs(mixed[:GRID_Y].contiguous(), cols)
    assert int((alone.view(torch.int32) != got[:GRID_Y].view(torch.int32)).sum()) > 0     # (the case can tell)
    _check_tail(any_sd, mixed, cols, got, np.array([0, 1, GRID_Y - 1, GRID_Y, where, r - 1]), cond=True, what="mixed")


# ---------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("hname", HANDLE_NAMES)
def test_row_blocks_on_dirty_workspaces(eng, wide_eng, any_eng, sd, any_sd, walk, hname):
    """0x00 / 0xFF / 0x7F / random workspaces on the multi-block path: identical outputs and status."""
    e, mask, _, width, scale = _handles(eng, wide_eng, any_eng, sd, any_sd)[hname]
    m, r = M_A, RB_A + 1
    rb = _rb(r, m)
    assert r > rb
    xz = _poses(walk, max(m, r + 17))
    cxz, rxz = xz[:m], xz[17:17 + r]
    xz_d = torch.from_numpy(xz).cuda()
    rows, cols = _pooled(r, width, scale, 71), _pooled(m, width, scale, 72)
    rs = torch.from_numpy(np.random.default_rng(3).integers(0, m, size=r).astype(np.int32))
    e.set_skip_mask(mask)
    try:
        score = e.score_all_pairs(rows, cols)
        thr = _quantile(score[:512], 0.99)
        total = int(e.score_above(rows, cols, thr, window=5, row0=17)[3][-1])
        cap = int(e.score_above(rows, cols, thr, window=5, row0=17)[3][rb]) + 3
        assert cap < total
        pos = e.pair_positives(score, row0=17, pose_xz=xz_d)[0]
        thr_t = _rank_of(pos, 2047)
        calls = {
            "topk": lambda: e.score_topk(rows, cols, k=16, window=5, row0=17, causal=True),
            "topk row_self": lambda: e.score_topk(rows, cols, k=1, window=3, row_self=rs),
            "mine negatives": lambda: e.score_mine(rows, cols, cxz, k=16, window=5, row0=17, causal=True),
            "mine positives": lambda: e.score_mine(rows, cols, cxz, k=4, positives=True, window=5, row0=17, row_pose=rxz),
            "above": lambda: e.score_above(rows, cols, thr, window=5, row0=17),
            "above capacity": lambda: _trim(e.score_above(rows, cols, thr, window=5, row0=17, capacity=cap)),
            "above count only": lambda: e.score_above(rows, cols, thr, window=5, row0=17, capacity=0),
            "positives": lambda: _sorted_positives(e.score_positives(rows, cols, row0=17, pose_xz=xz_d)),
            "counts": lambda: e.score_threshold_counts(rows, cols, thr_t[0], row0=17, pose_xz=xz_d, rank=thr_t[1]),
        }
        for what, fn in calls.items():
            _check_all_patterns(e, fn, (hname, what))
    finally:
        e.set_skip_mask(0)


def _sorted_positives(res):
    return torch.sort(res[0].view(torch.int32))[0], res[1]


def test_mining_on_dirty_workspaces(eng, walk):
    """score_mine on the production handle (fused, one launch): no test checked mining this way before."""
    r, m = 3000, M_A
    xz = _poses(walk, max(m, r + 900))
    cxz, rxz = xz[:m], xz[900:900 + r] + 0.5
    rows, cols = _pooled(r, 32, 3.0, 81), _pooled(m, 32, 3.0, 82)
    rs = torch.from_numpy(np.random.default_rng(4).integers(0, m, size=r).astype(np.int32))
    for k, pos, causal, kw in ((1, False, False, {}), (16, False, True, dict(row0=900)), (4, True, False, dict(row_pose=rxz)),
                               (16, True, True, dict(row_self=rs))):
        _check_all_patterns(eng, lambda: eng.score_mine(rows, cols, cxz, k=k, positives=pos, window=5, causal=causal, **kw),
                            ("mine", k, pos, causal))


# ---------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("hname", ["tuned, bit 13", "any-shape"])
def test_no_matrix_on_the_fallback_handles(eng, wide_eng, any_eng, sd, any_sd, walk, hname):
    """20 000 x 20 000: every epilogue's workspace and the peak memory a call adds stay below 0.1 of the matrix."""
    e, mask, _, width, scale = _handles(eng, wide_eng, any_eng, sd, any_sd)[hname]
    n = 20000
    matrix = 4 * n * n
    pooled = _pooled(n, width, scale, 91)
    xz_d = torch.from_numpy(_poses(walk, n)).cuda()
    thr = np.linspace(0.05, 0.95, 2047).astype(np.float32)
    calls = {
        "topk": lambda: e.score_topk(pooled, pooled, k=16, window=50, causal=True),
        "mine": lambda: e.score_mine(pooled, pooled, xz_d, k=16, window=50),
        "above": lambda: e.score_above(pooled, pooled, 0.999, window=50, causal=True, capacity=1 << 20),
        "positives": lambda: e.score_positives(pooled, pooled, pose_xz=xz_d),
        "counts": lambda: e.score_threshold_counts(pooled, pooled, thr, pose_xz=xz_d),
    }
    e.set_skip_mask(mask)                                # (the workspace sizes depend on the mask too)
    try:
        for ws in (e.score_topk_workspace_bytes(n, n, 16, causal=True), e.score_mine_workspace_bytes(n, n, 16),
                   e.score_mine_workspace_bytes(n, n, 16, positives=True), e.score_above_workspace_bytes(n, n),
                   e.score_positives_workspace_bytes(n, n), e.score_threshold_counts_workspace_bytes(n, n, 2047)):
            assert 0 < ws < 0.1 * matrix, ws
        for what, fn in calls.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            assert peak < 0.1 * matrix, (hname, what, peak)
            del out
    finally:
        e.set_skip_mask(0)
