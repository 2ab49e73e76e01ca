"""sgpr_seq_rows_above / sgpr_score_seq_above / sgpr_score_seq_positives / sgpr_score_seq_threshold_counts on the GPU:
the resident form against the NumPy reference (tests/seq_above_ref.py) bit for bit, the pooled form against
score_all_pairs -> seq_rows_above and -> seq_filter -> rows_above on the same rectangle (one block and several, on every
kind of handle), dirty workspaces, the pooled evaluation against the matrix kernels on Q, the place database online
against one offline call, and the two command-line tools."""
import ctypes
import os

import numpy as np
import pytest
import torch

import score_ref
import seq_above_ref
import seq_ref
from test_gpu_row_blocks import M_A, RB_A, _rows_quantity, _scale_row
from test_gpu_score_range import _any_shape, _wide_checkpoint
from test_gpu_seq import DIRECTIONS, _equal, _flags, _pooled, _scores, _seq_rb
from test_gpu_stateless import _check_all_patterns

pytestmark = pytest.mark.gpu

INF = float("inf")


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


def _host(got):
    return tuple(g.cpu().numpy() for g in got)


def _same(got, want, what, n=None):
    """(rows, cols, values, dirs, row_ptr) of the device against the reference's: the first n pairs (default all of
    them) and the whole row pointer, values by their bits"""
    rows, cols, vals, dirs, row_ptr = _host(got)
    wr, wc, wv, wd, wp = want
    n = wr.size if n is None else n
    assert np.array_equal(row_ptr, wp), (what, "row_ptr")
    assert rows.size >= n and cols.size >= n and vals.size >= n and dirs.size >= n, (what, rows.size, n)
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and dirs.dtype == np.uint8 and row_ptr.dtype == np.int64
    assert np.array_equal(rows[:n], wr[:n]) and np.array_equal(cols[:n], wc[:n]), (what, "rows / cols")
    assert np.array_equal(vals[:n].view(np.uint32), wv[:n].view(np.uint32)), (what, "values")
    assert np.array_equal(dirs[:n], wd[:n]), (what, "dirs")


# ------------------------------------------------------------------------------------------------- 1. the resident form
# the edges of the tile (32 x 256) and of the 64-column segment; (70, 300) with a strided ld
SHAPES = [(1, 1, 0), (5, 7, 0), (3, 64, 0), (3, 65, 0), (37, 131, 0), (70, 300, 5), (33, 255, 0), (33, 257, 0), (33, 515, 0)]
LENGTHS = (1, 2, 8, 32)


def _modes(r, m, seed):
    perm = np.random.default_rng(seed).permutation(max(r, m))[:r].astype(np.int32) % m
    return [dict(window=-1), dict(window=0), dict(window=10), dict(window=10, causal=True), dict(window=-1, causal=True),
            dict(window=10, row_self=perm), dict(window=0, causal=True, row_self=perm), dict(window=10, row0=4),
            dict(window=0, row0=4, causal=True)]


def _repeated_value(q, ok):
    """a finite value that occurs more than once among the eligible entries of q (or, none does, any of them)"""
    v = q[ok & np.isfinite(q)]
    if v.size == 0:
        return np.float32(0.5), 0
    u, n = np.unique(v, return_counts=True)
    j = int(np.argmax(n > 1)) if (n > 1).any() else u.size // 2
    return np.float32(u[j]), int(n[j])


def _raw_call(eng, dev, ld, ctx, L, flags, thr, mode, cap, want_row_ptr, want_dirs):
    """sgpr_seq_rows_above through ctypes, with d_row_ptr and d_dirs NULL on request"""
    from sg_pr_amd.engine import _ptr
    r, m = dev.shape
    rs = mode.get("row_self")
    rs = None if rs is None else torch.from_numpy(rs).cuda()
    n = max(cap, 1)
    out_r = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    out_c = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    out_v = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    out_d = torch.full((n,), 9, dtype=torch.uint8, device="cuda") if want_dirs else None
    row_ptr = torch.full((r - ctx + 1,), -7, dtype=torch.int64, device="cuda") if want_row_ptr else None
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws_bytes = eng.seq_rows_above_workspace_bytes(r, m, ctx)
    ws = eng._ws(ws_bytes)
    null = cap == 0
    rc = eng.lib.sgpr_seq_rows_above(eng._h, _ptr(dev), r, m, ld, ctx, _ptr(rs), int(mode.get("row0", 0)),
                                     int(mode.get("window", -1)), flags | (1 if mode.get("causal") else 0), L, float(thr),
                                     None if null else _ptr(out_r), None if null else _ptr(out_c),
                                     None if null else _ptr(out_v), None if null else _ptr(out_d), cap, _ptr(row_ptr),
                                     _ptr(count), _ptr(ws), ws_bytes, eng._stream())
    eng._check(rc)
    torch.cuda.synchronize()
    return out_r, out_c, out_v, out_d, row_ptr, int(count.item())


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_resident_form_equals_the_reference(eng, shape):
    r, m, pad = shape
    host = _scores(r, m, 7 * r + m, ld=m + pad)
    dev = torch.from_numpy(host).cuda()[:, :m]               # ld = m + pad: read in place
    finite = np.where(np.isinf(host), np.float32(0.25), host)
    dev_finite = torch.from_numpy(finite).cuda()[:, :m]
    modes = _modes(r, m, r + m)
    step, repeated, nonempty = 0, 0, 0
    for L in LENGTHS:
        for reverse in DIRECTIONS:
            fl = _flags(reverse)
            q_all, d_all = seq_ref.seq_filter(host[:, :m], L, 0, **fl)
            for ctx in sorted({0, min(L - 1, r), r - 1, r}):
                q, d = q_all[ctx:], d_all[ctx:]
                for j in range(3):                            # three of the nine eligibility modes per combination
                    mode = modes[(step + 3 * j) % len(modes)]
                    step += 1
                    ok = seq_above_ref.eligible(r, m, ctx, mode.get("window", -1), mode.get("row0", 0),
                                                mode.get("causal", False), mode.get("row_self"))
                    dup, n_dup = _repeated_value(q, ok)
                    repeated += n_dup > 1
                    for thr in (-INF, INF, dup):
                        want = seq_above_ref.select(q, d, ok, thr)
                        what = (shape, L, reverse, ctx, mode, float(thr))
                        got = eng.seq_rows_above(dev, L, thr, context=ctx, reverse=reverse, **mode)
                        assert got[0].numel() == want[0].size, what
                        _same(got, want, what)
                        nonempty += want[0].size > 0
                    if n_dup > 1:                             # >= and > differ there
                        above = np.nextafter(dup, np.float32(INF))
                        assert seq_above_ref.select(q, d, ok, above)[0].size < seq_above_ref.select(q, d, ok, dup)[0].size
                    # capacity: exact, three short, one (a prefix of the same order), and counting only
                    want = seq_above_ref.select(q, d, ok, dup)
                    total = want[0].size
                    for cap in sorted({total, max(total - 3, 0), 1, 0}):
                        got = eng.seq_rows_above(dev, L, dup, context=ctx, reverse=reverse, capacity=cap, **mode)
                        assert got[0].numel() == cap
                        _same(got, want, (shape, L, reverse, ctx, mode, "capacity", cap), n=min(cap, total))
            # a threshold above every value (the +-inf entries replaced): count 0, an all-zero row pointer
            qf, df = seq_ref.seq_filter(finite[:, :m], L, 0, **fl)
            top = np.nextafter(np.float32(np.nanmax(qf)), np.float32(INF)) if not np.isnan(qf).all() else np.float32(0)
            got = eng.seq_rows_above(dev_finite, L, top, reverse=reverse, window=-1)
            assert got[0].numel() == 0 and not got[4].any() and got[4].numel() == r + 1
            # row_ptr and dirs omitted, the arrays NULL with capacity 0 (the raw call)
            mode = modes[step % len(modes)]
            ok = seq_above_ref.eligible(r, m, 0, mode.get("window", -1), mode.get("row0", 0), mode.get("causal", False),
                                        mode.get("row_self"))
            thr = _repeated_value(q_all, ok)[0]
            want = seq_above_ref.select(q_all, d_all, ok, thr)
            total = want[0].size
            flags = (2 if fl["forward"] else 0) | (4 if fl["reverse"] else 0)
            ld = m + pad if r > 1 else m
            for want_rp, want_d, cap in ((False, False, total), (True, False, total), (False, True, total), (False, False, 0),
                                         (True, True, 0)):
                o_r, o_c, o_v, o_d, rp, n = _raw_call(eng, dev, ld, 0, L, flags, thr, mode, cap, want_rp, want_d)
                what = (shape, L, reverse, mode, "raw", want_rp, want_d, cap)
                assert n == total, what
                if want_rp:
                    assert np.array_equal(rp.cpu().numpy(), want[4]), what
                k = min(cap, total)
                assert np.array_equal(o_r.cpu().numpy()[:k], want[0][:k]) and np.array_equal(o_c.cpu().numpy()[:k], want[1][:k])
                assert np.array_equal(o_v.cpu().numpy()[:k].view(np.uint32), want[2][:k].view(np.uint32)), what
                if want_d:
                    assert np.array_equal(o_d.cpu().numpy()[:k], want[3][:k]), what
                if cap > total or cap == 0:                   # nothing written past the count
                    assert (o_r[k:] == -7).all() and (o_v[k:] == -7.0).all(), what
    assert nonempty > 0
    if r > 30:
        assert repeated > 0                                   # a value that occurs more than once was thresholded
    # two calls return identical bytes
    a = eng.seq_rows_above(dev, 8, 0.5, window=0, reverse="both")
    b = eng.seq_rows_above(dev, 8, 0.5, window=0, reverse="both")
    _equal(a, b, "two calls")
    eng.check_status()


def test_row_self_outside_the_columns_is_reported(eng):
    from sg_pr_amd.engine import SgprError
    dev = torch.from_numpy(_scores(5, 7, 1)).cuda()
    eng.seq_rows_above(dev, 2, 0.5, window=0, row_self=np.array([0, 1, 7, 3, 4], dtype=np.int32))
    with pytest.raises(SgprError):
        eng.check_status()
    eng.check_status()                                        # reported once, then clean


# ------------------------------------------------------------------------------------------------- 2. the pooled form
def _by_filter(e, score, L, thr, window=-1, row0=0, causal=False, row_self=None, context=0, reverse="both"):
    """seq_filter -> rows_above on Q, dirs gathered from the filter's dir"""
    q, d = e.seq_filter(score, L, context=context, reverse=reverse, want_dir=True)
    rs = None if row_self is None else row_self[context:]
    rows, cols, vals, row_ptr = e.rows_above(q, thr, window=window, row0=row0 + context, causal=causal, row_self=rs)
    return rows, cols, vals, d[rows.long(), cols.long()], row_ptr


@pytest.mark.parametrize("shape", [(37, 131), (300, 517)])
def test_pooled_equals_both_matrix_routes(eng, shape):
    r, m = shape
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(r).permutation(m)[:r].astype(np.int32))
    modes = [dict(window=-1), dict(window=0), dict(window=50), dict(window=50, causal=True), dict(window=-1, causal=True),
             dict(window=10, row_self=perm), dict(window=10, causal=True, row_self=perm), dict(window=50, row0=120),
             dict(window=0, row0=120, causal=True)]
    n = 0
    for L in (1, 2, 8, 32):
        for ctx in sorted({0, L - 1}):
            q = eng.seq_filter(score, L, context=ctx, reverse="both")
            for j, mode in enumerate(modes):
                reverse = DIRECTIONS[(j + n) % 3]
                thr = (float(q.flatten().kthvalue(int(0.9 * q.numel()))[0]), -INF, INF, 0.5)[(j + n) % 4]
                kw = dict(context=ctx, reverse=reverse, **mode)
                got = eng.score_seq_above(rows, cols, L, thr, **kw)
                _equal(got, eng.seq_rows_above(score, L, thr, **kw), (shape, L, thr, kw))
                _equal(got, _by_filter(eng, score, L, thr, **kw), (shape, L, thr, kw, "filter route"))
                assert got[4].shape == (r - ctx + 1,) and int(got[4][-1]) == got[0].numel()
            n += 1
    thr = float(eng.seq_filter(score, 8).flatten().kthvalue(int(0.9 * r * m))[0])
    full = eng.score_seq_above(rows, cols, 8, thr, window=0, context=7)
    total = full[0].numel()
    assert total > 100 and full[3].any() and not full[3].all()            # both directions are taken somewhere
    for cap in (total, total - 3, 1, 0):
        got = eng.score_seq_above(rows, cols, 8, thr, window=0, context=7, capacity=cap)
        _equal(tuple(g[:min(cap, total)] for g in got[:4]) + (got[4],), tuple(f[:min(cap, total)] for f in full[:4]) + (full[4],),
               ("capacity", cap))
    # empty calls: context == R, no columns, no rows
    for kw, n_ptr in ((dict(context=r), 1), (dict(context=2), r - 1)):
        c = cols if kw["context"] == r else cols[:0]
        got = eng.score_seq_above(rows, c, 8, 0.5, **kw)
        assert got[0].numel() == 0 and got[4].shape == (n_ptr,) and not got[4].any()
        got = eng.seq_rows_above(score[:, :c.shape[0]], 8, 0.5, **kw)
        assert got[0].numel() == 0 and got[4].shape == (n_ptr,) and not got[4].any()
    got = eng.score_seq_above(rows[:0], cols, 8, 0.5)
    assert got[0].numel() == 0 and got[4].tolist() == [0]
    eng.check_status()


def test_length_one_forward_equals_score_above(eng):
    rows, cols = _pooled(300, 32, 3.0, 1), _pooled(517, 32, 3.0, 2)
    for window, causal in ((-1, False), (50, True)):
        want = eng.score_above(rows, cols, 0.8, window=window, row0=3, causal=causal)
        got = eng.score_seq_above(rows, cols, 1, 0.8, window=window, row0=3, causal=causal, reverse=False)
        _equal(got[:3] + got[4:], want, ("L = 1", window, causal))
        assert not got[3].any()


# ------------------------------------------------------------------------------------------------- 3. several blocks
BLOCK_CASES = [(M_A, RB_A + 1, 8), (262144, 150, 32)]


def _threshold_at_rank(q, fraction=0.01):
    """the value that about `fraction` of the entries of q reach, read off at a fixed rank"""
    flat = q.flatten()
    return float(flat.kthvalue(flat.numel() - int(flat.numel() * fraction))[0])


def _blocks_equal(e, rows, cols, L, rb, kws, what):
    score = e.score_all_pairs(rows, cols)
    thr = _threshold_at_rank(e.seq_filter(score, L, reverse="both"))
    for kw in kws:
        got = e.score_seq_above(rows, cols, L, thr, **kw)
        want = e.seq_rows_above(score, L, thr, **kw)
        _equal(got, want, (what, kw))
        rp = got[4]
        assert (rp[1:] >= rp[:-1]).all() and int(rp[-1]) == got[0].numel() > 0
        edge = int(rp[max(rb - kw.get("context", 0), 0)])             # the row pointer continues across the blocks:
        assert int(rp[-1]) > edge and (edge > 0 or kw.get("causal"))   # pairs on both sides of the first block's end
    return score, thr


@pytest.mark.parametrize("case", BLOCK_CASES, ids=["rb+1", "thin"])
def test_several_blocks_tuned_handle(eng, case):
    m, r, L = case
    rb = _seq_rb(r, m, L)
    assert rb < r                                              # more than one block runs
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    perm = torch.from_numpy(np.random.default_rng(r).integers(0, m, size=r).astype(np.int32))
    _blocks_equal(eng, rows, cols, L, rb,
                  (dict(window=50, context=L - 1), dict(window=5, row0=7, causal=True, reverse=True),
                   dict(window=10, row_self=perm, reverse=False, context=3)), case)
    eng.check_status()


def test_several_blocks_wide_checkpoint(sd):
    from sg_pr_amd import engine
    m, r, L = M_A, RB_A + 1, 8
    wide = engine.Engine(_wide_checkpoint(sd), device=0)
    try:
        assert not wide.uses_f16_planes()
        rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
        _blocks_equal(wide, rows, cols, L, _seq_rb(r, m, L), (dict(window=50, context=L - 1),), "wide checkpoint")
        wide.check_status()
    finally:
        wide.close()


def test_several_blocks_any_shape():
    m, r, L = M_A, RB_A + 1, 8
    any_eng = _any_shape(_any_shape())
    try:
        assert any_eng.any_shape
        rows, cols = _pooled(r, 48, 1.0, r + 1), _pooled(m, 48, 1.0, m + 1)
        _blocks_equal(any_eng, rows, cols, L, _seq_rb(r, m, L), (dict(window=50, causal=True, context=2),), "any-shape")
        any_eng.check_status()
    finally:
        any_eng.close()


def test_f16_range_is_the_calls(eng, sd):
    """One row far outside the f16 range in the last block only: every block takes the datapath score_all_pairs takes on
    the whole rectangle (test_gpu_seq.test_f16_range_is_the_calls' construction)."""
    m, L = M_A, 8                                            # (few rows per block: the host's range quantities cost per row)
    rb = _seq_rb(1 << 30, m, L)
    r = rb + 37
    assert _seq_rb(r, m, L) == rb < r
    rows, cols = _pooled(r, 32, 1.0, 41), _pooled(m, 32, 1.0, 42)
    rn, cn = rows.cpu().numpy(), cols.cpu().numpy()
    thr = score_ref.F16_SAFE
    assert _rows_quantity(sd, rn, cn, "bound", score_ref.TUNED_K) < 0.97 * thr
    where = r - 3
    rows[where] *= _scale_row(sd, rn[where:where + 1], cn, "bound", 1.03 * thr, score_ref.TUNED_K)
    score = eng.score_all_pairs(rows, cols)
    alone = eng.score_all_pairs(rows[:rb].contiguous(), cols)
    assert int((alone.view(torch.int32) != score[:rb].view(torch.int32)).sum()) > 0   # the case can tell
    cut = _threshold_at_rank(eng.seq_filter(score, L, reverse="both"), 0.001)
    for kw in (dict(window=-1, context=L - 1), dict(window=5, row0=5, causal=True, reverse=True)):
        got = eng.score_seq_above(rows, cols, L, cut, **kw)
        _equal(got, eng.seq_rows_above(score, L, cut, **kw), ("mixed range", kw))
        assert got[0].numel() > 0
    xz = _circle(max(r, m))
    _eval_equal(eng, rows, cols, L, xz=xz, context=L - 1, reverse="both", what="mixed range", full=False)


# ------------------------------------------------------------------------------------------------- 4. statelessness
def test_dirty_workspaces(eng):
    rows, cols = _pooled(300, 32, 3.0, 5), _pooled(4541, 32, 3.0, 6)
    score = torch.from_numpy(_scores(300, 4541, 13)).cuda()
    xz = _circle(4541)
    cut = _threshold_at_rank(eng.seq_filter(eng.score_all_pairs(rows, cols), 8, reverse="both"))
    base = _check_all_patterns(eng, lambda: eng.score_seq_above(rows, cols, 8, cut, window=50, causal=True, context=7),
                               "score_seq_above")
    assert base[0].size > 100
    base = _check_all_patterns(eng, lambda: eng.score_seq_above(rows, cols, 32, 0.5, window=50, reverse=True, capacity=5),
                               "score_seq_above, capacity")
    assert base[4][-1] > 5
    _check_all_patterns(eng, lambda: eng.seq_rows_above(score, 8, 0.75, window=10, reverse="both"), "seq_rows_above")
    _check_all_patterns(eng, lambda: torch.sort(eng.score_seq_positives(rows, cols, 8, pose_xz=xz, context=7)[0])[0],
                        "score_seq_positives")
    thr = np.linspace(0.1, 0.9, 9, dtype=np.float32)
    _check_all_patterns(eng, lambda: torch.from_numpy(eng.score_seq_threshold_counts(rows, cols, 8, thr, pose_xz=xz,
                                                                                     context=7)[0]),
                        "score_seq_threshold_counts")


# ------------------------------------------------------------------------------------------------- 5. pooled evaluation
def _circle(n, radius=40.0, step=0.11):
    """planar poses of a trajectory that drives a circle again and again: every place is revisited each 57 frames"""
    t = np.arange(n) * step
    return torch.from_numpy(np.stack((radius * np.cos(t), radius * np.sin(t)), axis=1)).cuda()


def _rank_of(pos, t):
    from sg_pr_amd import metrics
    u, mult = metrics.distinct_counts(pos.cpu().numpy())
    above = np.concatenate((np.cumsum(mult[::-1])[::-1], [0])).astype(np.int64)
    step = max(1, -(-u.size // t))
    return u[::step], (u, step, above)


def _eval_equal(e, rows, cols, L, row0=0, xz=None, gt=None, context=0, reverse="both", what="", full=True):
    """score_seq_positives / score_seq_threshold_counts / (full) pr_roc_seq_pooled against the matrix kernels on
    Q = seq_filter(score_all_pairs)"""
    from sg_pr_amd import metrics
    q = e.seq_filter(e.score_all_pairs(rows, cols), L, context=context, reverse=reverse)
    want, wbad = e.pair_positives(q, row0=row0 + context, pose_xz=xz, gt=gt)
    got, gbad = e.score_seq_positives(rows, cols, L, row0=row0, pose_xz=xz, gt=gt, context=context, reverse=reverse)
    assert gbad == wbad and want.numel() > 0, what
    assert torch.equal(torch.sort(got.view(torch.int32))[0], torch.sort(want.view(torch.int32))[0]), what
    for t in (1, 7, e.MAX_POOLED_THRESHOLDS) if full else (7,):
        thr, rank = _rank_of(want, t)
        for rk in (None, rank) if full else (rank,):
            w = e.pair_threshold_counts(q, thr, row0=row0 + context, pose_xz=xz, gt=gt, rank=rk)
            g = e.score_seq_threshold_counts(rows, cols, L, thr, row0=row0, pose_xz=xz, gt=gt, rank=rk, context=context,
                                             reverse=reverse)
            assert np.array_equal(g[0], w[0]) and g[1:] == w[1:], (what, t, rk is not None)
            assert int(w[0].sum()) > 0
    if not full:
        return None
    f1, auc, _ = metrics.pr_roc_seq_pooled(e, rows, cols, L, pose_xz=xz, gt=gt, row0=row0, context=context, reverse=reverse)
    f1m, aucm, _ = metrics.pr_roc_device(e, q, pose_xz=xz, gt=gt, row0=row0 + context)
    assert f1 == f1m and auc == aucm and 0.0 < f1 <= 1.0, (what, f1, f1m, auc, aucm)
    assert metrics.f1_max_seq_pooled(e, rows, cols, L, pose_xz=xz, gt=gt, row0=row0, context=context, reverse=reverse)[0] == f1
    assert metrics.roc_auc_seq_pooled(e, rows, cols, L, pose_xz=xz, gt=gt, row0=row0, context=context, reverse=reverse) == auc
    return f1, auc


def _labels(r, m, seed, keep=0.2):
    """int8 labels: one cell in twenty ignored (-1), a fraction 0.9 keep of them positive"""
    g = torch.Generator().manual_seed(seed)
    gt = (torch.randint(0, 20, (r, m), generator=g) - 1).clamp(max=1).to(torch.int8)    # -1 / 0 / 1
    gt[gt == 1] = torch.where(torch.rand(int((gt == 1).sum()), generator=g) < keep, 1, 0).to(torch.int8)
    return gt


def test_pooled_evaluation_one_block(eng):
    rows, cols = _pooled(300, 32, 3.0, 11), _pooled(517, 32, 3.0, 12)
    xz = _circle(517)
    n = 0
    for L in (1, 2, 8, 32):
        for ctx in sorted({0, L - 1}):
            reverse = DIRECTIONS[n % 3]
            _eval_equal(eng, rows, cols, L, row0=40, xz=xz, context=ctx, reverse=reverse, what=("poses", L, ctx))
            _eval_equal(eng, rows, cols, L, gt=_labels(300 - ctx, 517, n), context=ctx, reverse=reverse, what=("gt", L, ctx))
            n += 1
    # empty calls
    for kw in (dict(context=300), dict(context=0, cols=cols[:0])):
        c = kw.pop("cols", cols)
        pos, bad = eng.score_seq_positives(rows, c, 8, pose_xz=xz, **kw)
        assert pos.numel() == 0 and bad == 0
        counts, bad, rs = eng.score_seq_threshold_counts(rows, c, 8, np.array([0.5], dtype=np.float32), pose_xz=xz, **kw)
        assert not counts.any() and bad == 0
    eng.check_status()


@pytest.mark.parametrize("kind", ["poses", "gt"])
def test_pooled_evaluation_several_blocks(eng, kind):
    m, r, L = M_A, RB_A + 1, 8
    assert _seq_rb(r, m, L) < r
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    if kind == "poses":
        _eval_equal(eng, rows, cols, L, row0=5, xz=_circle(m), context=L - 1, reverse="both", what="blocks, poses")
    else:
        _eval_equal(eng, rows, cols, L, gt=_labels(r - 3, m, 5, keep=0.002), context=3, reverse=True, what="blocks, gt",
                    full=False)              # (F1 of labels that ignore the scores is flat: refining it takes many passes)
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 6. online = offline
@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_place_database_online_equals_offline(model):
    """query_seq_above before every append (causal, L = 8; window 10 >= L - 1) against one score_seq_above call over the
    whole sequence."""
    from sg_pr_amd.place_db import PlaceDatabase
    n, L, window = 120, 8, 10
    pooled = _pooled(n, 32, 3.0, 77)
    e = model.engine()
    thr = _threshold_at_rank(e.seq_filter(e.score_all_pairs(pooled, pooled), L, reverse="both"), 0.2)
    db = PlaceDatabase(model, capacity=4)
    got, base = [], 0
    for t in range(n):
        rows, ids, vals, dirs, row_ptr = db.query_seq_above(None, None, L, thr, window=window, causal=True,
                                                            pooled=pooled[t:t + 1])
        assert row_ptr.tolist() == [0, rows.numel()] and not rows.any()
        got.append((rows + t, ids, vals, dirs))
        db.append_pooled(pooled[t:t + 1])
    online = tuple(torch.cat([g[j] for g in got]) for j in range(4))
    offline = e.score_seq_above(pooled, pooled, L, thr, window=window, causal=True)
    assert offline[0].numel() > 50 and offline[3].any() and not offline[3].all()
    _equal(online, offline[:4], "online / offline")
    counts = torch.tensor([g[0].numel() for g in got])
    assert torch.equal(torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0))), offline[4].cpu())
    # a run of members, and the model's route to the same call
    want = e.score_seq_above(pooled, pooled, L, thr, window=window)
    run = db.query_ids_seq_above(40, 30, L, thr, window=window)
    lo, hi = int(want[4][40]), int(want[4][70])
    _equal(run[:4], (want[0][lo:hi] - 40,) + tuple(w[lo:hi] for w in want[1:4]), "query_ids_seq_above")
    assert torch.equal(run[4], want[4][40:71] - lo)
    _equal(model.loop_closures_above(pooled, pooled, thr, window=window, seq_len=L), want, "loop_closures_above seq_len")
    _equal(model.loop_closures_above(pooled, pooled, thr, window=window), e.score_above(pooled, pooled, thr, window=window),
           "loop_closures_above seq_len = 1")
    xz = _circle(n)
    assert model.evaluate_pooled(pooled, pooled, pose_xz=xz, seq_len=L)[:2] == \
        _eval_equal(e, pooled, pooled, L, xz=xz, what="evaluate_pooled")
    from sg_pr_amd import metrics
    assert model.evaluate_pooled(pooled, pooled, pose_xz=xz) == metrics.pr_roc_pooled(e, pooled, pooled, pose_xz=xz)
    e.check_status()


# ------------------------------------------------------------------------------------------------- 7. the tools
def test_command_line_tools(model, tmp_path, ckpt_path):
    from sg_pr_amd import graph_store, place_db, synth
    n = 120
    centers, labels, _, poses = synth.world_sequence(n, 100, seed=4)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(n)])
    os.makedirs(tmp_path / "eva")
    seq.save(str(tmp_path / "eva" / "07_packed.npz"))
    cfg = tmp_path / "config.yml"
    cfg.write_text("""
common: {model: "%s", cuda: "0", batch_size: 128, p_thresh: 3, graph_pairs_dir: "%s", pair_list_dir: '%s'}
arch: {keep_node: 1, filters_1: 64, filters_2: 64, filters_3: 32, tensor_neurons: 16, bottle_neck_neurons: 16, K: 10}
train: {epochs: 500, train_sequences: ['00'], eval_sequences: ["08"], dropout: 0, learning_rate: 0.001,
        weight_decay: 0.0005, gpu: 0, logdir: "./logs_k10", node_num: 100}
eva_batch: {sequences: ["07"], output_path: "%s", show: False}
eva_pair: {pair_file: ["a.json", "b.json"]}
""" % (ckpt_path, tmp_path / "graphs", tmp_path, tmp_path / "eva"))
    eva = tmp_path / "eva"
    place_db.main([str(cfg), "--window", "10", "--threshold", "0.9"])                # as before: no sequence file
    plain = {k: v.copy() for k, v in np.load(eva / "07_above.npz").items()}
    assert not os.path.exists(eva / "07_seq_above.npz")
    place_db.main([str(cfg), "--window", "10", "--threshold", "0.9", "--seq-len", "8"])
    again = np.load(eva / "07_above.npz")
    assert sorted(again.files) == sorted(plain) == ["cols", "precision", "recall", "rows", "scores"]
    for k in plain:
        assert again[k].dtype == plain[k].dtype and again[k].tobytes() == plain[k].tobytes(), k   # the single-scan result
    z = np.load(eva / "07_seq_above.npz")
    assert sorted(z.files) == ["cols", "dirs", "precision", "recall", "rows", "scores", "seq_len"]
    eng = model.engine()
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    rows, cols, vals, dirs, _ = eng.score_seq_above(pooled, pooled, 8, 0.9, window=10)
    assert rows.numel() > 0 and int(z["seq_len"]) == 8
    assert np.array_equal(z["rows"], rows.cpu().numpy()) and np.array_equal(z["cols"], cols.cpu().numpy())
    assert np.array_equal(z["scores"].view(np.uint32), vals.cpu().numpy().view(np.uint32))
    assert np.array_equal(z["dirs"], dirs.cpu().numpy()) and z["dirs"].dtype == np.uint8
    assert 0.0 <= float(z["precision"]) <= 1.0 and 0.0 <= float(z["recall"]) <= 1.0

    graph_store.main([str(cfg), "--seq-len", "8"])
    with open(eva / "07_seq_F1_max.txt") as f:
        matrix_f1 = f.read()
    matrix_lc = np.load(eva / "07_seq_loop_closures.npy")
    os.remove(eva / "07_seq_F1_max.txt")
    os.remove(eva / "07_seq_loop_closures.npy")
    graph_store.main([str(cfg), "--no-matrix", "--seq-len", "8"])
    with open(eva / "07_seq_F1_max.txt") as f:
        assert f.read() == matrix_f1                                                  # the same number, digit for digit
    assert np.array_equal(np.load(eva / "07_seq_loop_closures.npy"), matrix_lc)
    r = graph_store.evaluate_all_pairs(model, seq, p_thresh=3.0, seq_len=8)
    p = graph_store.evaluate_seq_pooled(model, seq, 8, "both", p_thresh=3.0)
    assert sorted(p) == ["seq_closure_dirs", "seq_closure_frames", "seq_closure_scores", "seq_f1_max", "seq_roc_auc"]
    assert p["seq_f1_max"] == r["seq_f1_max"] == float(matrix_f1) and p["seq_roc_auc"] == r["seq_roc_auc"]
    _equal((p["seq_closure_scores"], p["seq_closure_frames"]), (r["seq_closure_scores"], r["seq_closure_frames"]), "closures")
    assert p["seq_closure_dirs"].shape == (n, 1) and p["seq_closure_dirs"].dtype == torch.uint8
    with pytest.raises(ValueError, match="keep_matrix"):
        graph_store.evaluate_all_pairs(model, seq, p_thresh=3.0, seq_len=8, keep_matrix=False)
    eng.check_status()
