"""sgpr_session_rows_above / sgpr_score_session_above on the GPU: the resident form against the NumPy reference
(tests/session_above_ref.py) bit for bit - rows, cols, values, codes, row_ptr, count - at the edges of the tile and of the
64-column segment, over the lengths, directions, context rows, path sets, minimum term counts, seams, windows, row frames,
thresholds and capacities; the two device identities; the pooled form on the tuned and the any-shape handle, across the
f16 range and across a block boundary with a row seam on either side; SG.loop_closures_above, the place database fed one
scan at a time, the place_db CLI and tools/session_above_bench.py."""
import os

import numpy as np
import pytest
import torch

import score_ref
import seq_path_ref
import session_above_ref as sar
import session_ref
from test_gpu_row_blocks import M_A, RB_A, _rows_quantity, _scale_row
from test_gpu_score_range import _any_shape
from test_gpu_seq import DIRECTIONS, LENGTHS, _equal, _flags, _pooled, _scores, _seq_rb
from test_gpu_seq_paths import _path_sets
from test_gpu_session import _row_tables, _tab

pytestmark = pytest.mark.gpu

INF = float("inf")
TR, TC = 32, 256                  # session_above_kernel's tile (SEQ_TR, SEQ_TC of sgpr_seq.hip): output rows x columns


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
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def _same(got, want, what, n=None):
    """(rows, cols, values, codes, row_ptr) of the device against the reference's: the first n pairs (default all of
    them) and the whole row pointer, values by their bits"""
    rows, cols, vals, codes, row_ptr = (g.cpu().numpy() for g in got)
    wr, wc, wv, wd, wp = want
    n = wr.size if n is None else n
    assert row_ptr.dtype == np.int64 and np.array_equal(row_ptr, wp), (what, "row_ptr")
    assert rows.size >= n and cols.size >= n and vals.size >= n and codes.size >= n, (what, rows.size, n)
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and codes.dtype == np.uint8 and vals.dtype == np.float32
    assert np.array_equal(rows[:n], wr[:n]) and np.array_equal(cols[:n], wc[:n]), (what, "rows / cols")
    assert np.array_equal(vals[:n].view(np.uint32), wv[:n].view(np.uint32)), (what, "values")
    assert np.array_equal(codes[:n], wd[:n]), (what, "codes")


def _col_tables(m):
    """column seams at 63 | 64 | 65 and 255 | 256 | 257 (either side of a segment's and of a tile's edge), at 1, M - 1 and
    M, an empty session, a table beginning [0, 0, ..]; one session"""
    return [None, _tab([63, 64, 65], m), _tab([255, 256, 257], m), _tab([1, m - 1, m], m), _tab([0, 64, 64, 256], m),
            _tab([65, m, m], m), _tab([0, 0, 255], m)]


def _raw_call(eng, dev, ld, ctx, L, flags, paths, rt, ct, mt, thr, mode, cap, want_row_ptr=True, want_codes=True):
    """sgpr_session_rows_above through ctypes on sentinel-filled outputs; the arrays NULL with capacity 0"""
    from sg_pr_amd.engine import _ptr
    r, m = dev.shape
    rs = mode.get("row_self")
    rs = None if rs is None else torch.from_numpy(rs).cuda()
    n = cap + 5
    out_r = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    out_c = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    out_v = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    out_d = torch.full((n,), 99, dtype=torch.uint8, device="cuda") if want_codes else None
    row_ptr = torch.full((r - ctx + 1,), -7, dtype=torch.int64, device="cuda") if want_row_ptr else None
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws_bytes = eng.session_rows_above_workspace_bytes(r, m, ctx)
    ws = eng._ws(ws_bytes)
    null = cap == 0
    tabs = []
    for t in (paths, rt, ct):
        t = None if t is None else np.ascontiguousarray(t, dtype=np.int32)
        tabs.append(t)
    args = []
    for t in tabs:
        args += [None, 0] if t is None else [t.ctypes.data, t.shape[0]]
    rc = eng.lib.sgpr_session_rows_above(eng._h, _ptr(dev), r, m, ld, ctx, _ptr(rs), int(mode.get("row0", 0)),
                                         int(mode.get("window", -1)), flags | (1 if mode.get("causal") else 0), L, *args,
                                         int(mt), float(thr), None if null else _ptr(out_r), None if null else _ptr(out_c),
                                         None if null else _ptr(out_v), None if null else _ptr(out_d), cap, _ptr(row_ptr),
                                         _ptr(count), _ptr(ws), ws_bytes, eng._stream())
    eng._check(rc)
    torch.cuda.synchronize()
    return out_r, out_c, out_v, out_d, row_ptr, int(count.item())


def _entry(q, ok):
    """a finite value of an eligible entry of q, one that occurs more than once if there is one"""
    v = q[ok & np.isfinite(q)]
    if v.size == 0:
        return np.float32(0.5)
    u, n = np.unique(v, return_counts=True)
    return np.float32(u[int(np.argmax(n > 1))] if (n > 1).any() else u[u.size // 2])


# ------------------------------------------------------------------------------------------------- 1. the resident form
# 1 x 1, the 64-column segment's and the 256-column tile's edges, more than one row tile, a third column tile; (70, 300)
# with a strided ld
SHAPES = [(1, 1, 0), (1, 63, 0), (1, 64, 0), (1, 65, 0), (TR + 1, TC - 1, 0), (TR + 1, TC, 0), (TR + 1, TC + 1, 0),
          (TR + 1, 2 * TC + 3, 0), (70, 300, 5)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_resident_form_equals_the_reference(eng, shape):
    r, m, pad = shape
    host = _scores(r, m, 11 * r + m, ld=m + pad)              # NaN, +-inf, -0.0 and repeated values among the entries
    dev = torch.from_numpy(host).cuda()[:, :m]               # ld = m + pad: read in place
    assert dev.stride(0) == m + pad or r == 1
    rng = np.random.default_rng(r * m)
    explicit = rng.integers(0, m, size=r).astype(np.int32)   # row frames anywhere in [0, M): other sessions too
    selfs = [dict(row0=0), dict(row0=7), dict(row0=m), dict(row_self=explicit)]
    n = nonempty = ineligible = capped = 0
    for L in LENGTHS:
        ctxs = sorted({0, min(1, r), min(L - 1, r), r - 1, r})
        for name, paths in _path_sets(L)[:3]:                 # the unit path, the 9-path set, the jump of 64
            for reverse in DIRECTIONS:
                ctx = ctxs[n % len(ctxs)]
                mt = sorted({1, min(2, L), L})[(n // 2) % len({1, min(2, L), L})]
                rt = _row_tables(r, ctx)[(n // 3) % 6]
                ct = _col_tables(m)[(n + 1) % 7]
                mode = dict(window=(-1, 0, 3)[(n // 2) % 3], causal=bool((n // 5) % 2), **selfs[(n // 4) % 4])
                table = None if (name == "unit" and n % 2) else paths      # no table: the unit diagonal
                n += 1
                fl = _flags(reverse)
                kw = dict(ctx=ctx, row_starts=rt, col_starts=ct, min_terms=mt, **fl)
                q, code, have = sar.fold(host[:, :m], table, L, **kw)
                ok = sar.eligible(r, m, ctx, have, ct, mode["window"], mode.get("row0", 0), mode["causal"],
                                  mode.get("row_self"))
                ineligible += int((~have).sum())
                what = (shape, L, name, reverse, ctx, mt, None if rt is None else rt.tolist(),
                        None if ct is None else ct.tolist(), {k: v for k, v in mode.items() if k != "row_self"})
                at = _entry(q, ok)
                ekw = dict(paths=table, row_sessions=rt, col_sessions=ct, min_terms=mt, context=ctx, reverse=reverse, **mode)
                counts = []
                for thr in (-INF, INF, np.nextafter(at, np.float32(-INF)), at, np.nextafter(at, np.float32(INF))):
                    want = sar.seq_above_ref.select(q, code, ok, thr)
                    got = eng.session_rows_above(dev, L, float(thr), **ekw)
                    assert got[0].numel() == want[0].size, (what, float(thr))
                    _same(got, want, (what, float(thr)))
                    counts.append(want[0].size)
                nonempty += counts[0] > 0
                assert counts[0] >= counts[2] >= counts[3] >= counts[4] >= counts[1]      # (+inf takes the +inf entries of Q)
                if n % 3 == 0:                                # capacity on sentinel-filled outputs (the raw call)
                    want = sar.seq_above_ref.select(q, code, ok, at)
                    total = want[0].size
                    flags = (2 if fl["forward"] else 0) | (4 if fl["reverse"] else 0)
                    ld = m + pad if r > 1 else m
                    for cap in sorted({0, 1, max(total - 1, 0), total}):
                        o_r, o_c, o_v, o_d, rp, cnt = _raw_call(eng, dev, ld, ctx, L, flags, table, rt, ct, mt, at, mode, cap)
                        k = min(cap, total)
                        assert cnt == total and np.array_equal(rp.cpu().numpy(), want[4]), (what, "capacity", cap)
                        _same((o_r[:k], o_c[:k], o_v[:k], o_d[:k], rp), want, (what, "capacity", cap), n=k)
                        assert (o_r[k:] == -7).all() and (o_c[k:] == -7).all() and (o_v[k:] == -7.0).all() and \
                            (o_d[k:] == 99).all(), (what, "past the count", cap)
                        capped += cap < total
                    # d_row_ptr and d_codes NULL
                    o_r, o_c, o_v, o_d, rp, cnt = _raw_call(eng, dev, ld, ctx, L, flags, table, rt, ct, mt, at, mode, total,
                                                            want_row_ptr=False, want_codes=False)
                    assert cnt == total and np.array_equal(o_c.cpu().numpy()[:total], want[1]), (what, "no row_ptr")
    assert nonempty > 0 and capped > 0
    if r > 1:
        assert ineligible > 0                                 # end points without a participating candidate occurred
    eng.check_status()                                        # every row frame lies in [0, M): nothing reported


def test_min_terms_one_is_session_filter_then_rows_above(eng):
    """min_terms = 1 with a finite threshold: session_filter + rows_above(window=-1), codes gathered"""
    r, m = 70, 300
    dev = torch.from_numpy(_scores(r, m, 31)).cuda()
    explicit = torch.from_numpy(np.random.default_rng(4).integers(0, m, size=r).astype(np.int32))
    n = 0
    for L in (1, 3, 8, 32):
        for name, paths in _path_sets(L)[:3]:
            for reverse in DIRECTIONS:
                ctx = (0, L - 1)[n % 2]
                rt, ct = _row_tables(r, ctx)[n % 6], _col_tables(m)[(n + 2) % 7]
                who = (dict(row0=0), dict(row0=9), dict(row_self=explicit))[n % 3]
                window, causal = (-1, 0, 3)[n % 3], bool(n % 2)
                n += 1
                q, c = eng.session_filter(dev, L, paths, row_sessions=rt, col_sessions=ct, window=window, context=ctx,
                                          reverse=reverse, want_code=True, **who)
                rs = who.get("row_self")
                rows, cols, vals, row_ptr = eng.rows_above(q, 0.5, window=-1, row0=who.get("row0", 0) + ctx, causal=causal,
                                                           row_self=None if rs is None else rs[ctx:])
                want = (rows, cols, vals, c[rows.long(), cols.long()], row_ptr)
                got = eng.session_rows_above(dev, L, 0.5, paths, row_sessions=rt, col_sessions=ct, min_terms=1,
                                             window=window, causal=causal, context=ctx, reverse=reverse, **who)
                _equal(got, want, (L, name, reverse, ctx, window, causal))
                assert got[0].numel() > 0
    eng.check_status()


def test_row_self_outside_the_columns_is_reported(eng):
    """row frames in another session raise nothing; a negative one and one at or past M raise the status bit - and the
    pairs are the reference's all the same"""
    from sg_pr_amd.engine import SgprError
    r, m, L = 9, 70, 3
    host = _scores(r, m, 2)
    dev = torch.from_numpy(host).cuda()
    ct = _tab([20, 64], m)
    for rs, raises in ((np.array([65, 3, 21, 69, 0, 19, 20, 64, 63], dtype=np.int32), False),
                       (np.array([65, 3, 21, -1, 0, 19, 20, 64, 63], dtype=np.int32), True),
                       (np.array([65, 3, 21, 69, 0, 19, m, 64, 63], dtype=np.int32), True),
                       (np.array([65, 3, -9, 69, 0, 19, m + 3, 64, 63], dtype=np.int32), True)):
        for causal in (False, True):
            want = sar.session_above(host, 0.5, None, L, ctx=2, forward=True, reverse=True, col_starts=ct, min_terms=2,
                                     window=5, causal=causal, row_self=rs)
            got = eng.session_rows_above(dev, L, 0.5, col_sessions=ct, min_terms=2, window=5, causal=causal, row_self=rs,
                                         context=2)
            _same(got, want, (rs.tolist(), causal))
            assert bool(((rs < 0) | (rs >= m)).any()) == raises
            if raises:
                with pytest.raises(SgprError):
                    eng.check_status()
            eng.check_status()                                # reported once, then clean


def test_two_streams_return_identical_bytes(eng):
    r, m = 70, 600
    dev = torch.from_numpy(_scores(r, m, 8)).cuda()
    nine = seq_path_ref.seq_paths(8, seq_path_ref.SLOPES)
    kw = dict(paths=nine, row_sessions=[0, 33], col_sessions=[0, 255, 256], min_terms=4, window=3, context=7)
    base = eng.session_rows_above(dev, 8, 0.5, **kw)
    n = base[0].numel()
    assert n > 100
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        a = eng.session_rows_above(dev, 8, 0.5, capacity=n, **kw)
    with torch.cuda.stream(sb):
        b = eng.session_rows_above(dev, 8, 0.5, capacity=n, **kw)
    sa.synchronize()
    sb.synchronize()
    _equal(a, base, "stream a")
    _equal(b, base, "stream b")
    _equal(eng.session_rows_above(dev, 8, 0.5, **kw), base, "two calls")


# ------------------------------------------------------------------------------------------------- 2. the pooled form
def _pooled_equals_resident(e, rows, cols, L, thr, kws, what, score=None):
    score = e.score_all_pairs(rows, cols) if score is None else score
    out = []
    for kw in kws:
        got = e.score_session_above(rows, cols, L, thr, **kw)
        _equal(got, e.session_rows_above(score, L, thr, **kw), (what, {k: v for k, v in kw.items() if k != "row_self"}))
        assert int(got[4][-1]) == got[0].numel()
        out.append(got)
    return out


def _quantile(e, score, L, keep=0.01):
    flat = e.seq_filter(score, L, reverse="both").flatten()
    flat = flat[torch.isfinite(flat)]
    return float(flat.kthvalue(flat.numel() - int(flat.numel() * keep))[0])


@pytest.mark.parametrize("handle", ["tuned", "any-shape"])
def test_pooled_equals_the_resident_form_and_the_reference(eng, handle):
    e = eng if handle == "tuned" else _any_shape(_any_shape())
    try:
        r, m = 37, 131
        width, scale = (32, 3.0) if handle == "tuned" else (48, 1.0)
        rows, cols = _pooled(r, width, scale, r), _pooled(m, width, scale, m)
        score = e.score_all_pairs(rows, cols)
        host = score.cpu().numpy()
        perm = np.random.default_rng(r).permutation(m)[:r].astype(np.int32)
        rt, ct = _tab([r // 3, r // 3 + 1, r - 1], r), _tab([1, 64, 64, m - 1, m], m)
        n = 0
        for L in (1, 2, 8, 32):
            for name, paths in _path_sets(L)[:3]:
                reverse = DIRECTIONS[n % 3]
                ctx = (0, 3, min(L - 1, r))[n % 3]
                mt = (1, min(2, L), L)[n % 3]
                mode = (dict(window=-1), dict(window=3, causal=True), dict(window=10, row_self=perm),
                        dict(window=5, row0=m - r))[n % 4]
                n += 1
                thr = (_quantile(e, score, L, 0.1), -INF, 0.5)[n % 3]
                kw = dict(paths=paths, row_sessions=rt, col_sessions=ct, min_terms=mt, context=ctx, reverse=reverse, **mode)
                got = _pooled_equals_resident(e, rows, cols, L, thr, (kw,), (handle, L, name), score=score)[0]
                want = sar.session_above(host, thr, paths, L, ctx=ctx, row_starts=rt, col_starts=ct, min_terms=mt,
                                         window=mode["window"], row0=mode.get("row0", 0), causal=mode.get("causal", False),
                                         row_self=mode.get("row_self"), **_flags(reverse))
                _same(got, want, (handle, L, name, mt, ctx))
        # empty calls: context == R, no columns, no rows
        for kw, n_ptr in ((dict(context=r), 1), (dict(context=2), r - 1)):
            c = cols if kw["context"] == r else cols[:0]
            got = e.score_session_above(rows, c, 8, 0.5, **kw)
            assert got[0].numel() == 0 and got[4].shape == (n_ptr,) and not got[4].any()
            got = e.session_rows_above(score[:, :c.shape[0]], 8, 0.5, **kw)
            assert got[0].numel() == 0 and got[4].shape == (n_ptr,) and not got[4].any()
        got = e.score_session_above(rows[:0], cols, 8, 0.5, min_terms=8)
        assert got[0].numel() == 0 and got[4].tolist() == [0]
        from sg_pr_amd.engine import SgprError
        for bad in (dict(min_terms=0), dict(min_terms=9), dict(col_sessions=[0, m + 1]), dict(row_sessions=[1])):
            with pytest.raises(SgprError):
                e.score_session_above(rows, cols, 8, 0.5, **bad)
        e.check_status()
    finally:
        if handle != "tuned":
            e.close()


def test_one_session_unit_path_is_score_seq_above(eng):
    rows, cols = _pooled(300, 32, 3.0, 1), _pooled(517, 32, 3.0, 2)
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(517)[:300].astype(np.int32))
    n = 0
    for L in (1, 8, 32):
        thr = _quantile(eng, score, L, 0.05)
        for elig in (dict(window=-1), dict(window=50, causal=True), dict(window=10, row0=3),
                     dict(window=10, row_self=perm, causal=True)):
            reverse = DIRECTIONS[n % 3]
            tables = (dict(), dict(row_sessions=[0], col_sessions=[0]))[n % 2]
            n += 1
            kw = dict(context=L - 1, reverse=reverse, **elig)
            want = eng.score_seq_above(rows, cols, L, thr, **kw)
            assert want[0].numel() > 0
            _equal(eng.score_session_above(rows, cols, L, thr, min_terms=1, **tables, **kw), want, ("one session", L, kw))
            _equal(eng.session_rows_above(score, L, thr, min_terms=1, **tables, **kw), want, ("resident", L, kw))
            assert eng.score_session_above_workspace_bytes(300, 517, L, 0, causal=elig.get("causal", False), context=L - 1,
                                                           reverse=reverse, n_row_sessions=1, n_col_sessions=1) == \
                eng.score_seq_above_workspace_bytes(300, 517, L, causal=elig.get("causal", False), context=L - 1,
                                                    reverse=reverse)
    eng.check_status()


def test_several_blocks_with_a_row_seam_either_side_of_the_boundary(eng):
    m, r, L = M_A, RB_A + 1, 8
    rb = _seq_rb(r, m, L)
    assert rb < r                                              # two blocks: rows 0 .. rb - 1 and rb .. r - 1
    rt, ct = _tab([rb - 1, rb + 1], r), _tab([m // 3, m // 3 + 300], m)
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    thr = _quantile(eng, score, L)
    perm = torch.from_numpy(np.random.default_rng(r).integers(0, m, size=r).astype(np.int32))
    ctx = L - 1
    kws = (dict(paths=nine, row_sessions=rt, col_sessions=ct, min_terms=1, window=50, context=ctx),
           dict(paths=nine, row_sessions=rt, col_sessions=ct, min_terms=2, window=50, context=ctx),
           dict(paths=None, row_sessions=rt, col_sessions=ct, min_terms=L, window=5, row0=7, causal=True, reverse=True),
           dict(paths=nine, row_sessions=rt, min_terms=3, window=10, causal=True, row_self=perm, reverse=False, context=3))
    got = _pooled_equals_resident(eng, rows, cols, L, thr, kws, "blocks", score=score)
    per_row = lambda g: (g[4][1:] - g[4][:-1]).cpu().numpy()
    one, two = per_row(got[0]), per_row(got[1])
    for row in (ctx, rb - 1, rb, r - 1):                      # a hit in the first and the last row of each block
        assert one[row - ctx] > 0, row
    # rows rb - 1 and rb + 1 start a session: one term, not eligible at min_terms = 2; row rb has two
    assert two[rb - 1 - ctx] == 0 and two[rb + 1 - ctx] == 0 and two[rb - ctx] > 0 and two[r - 1 - ctx] > 0
    cap = got[0][0].numel() - 3                                # capacity cuts inside the last block: counts stay exact
    cut = eng.score_session_above(rows, cols, L, thr, capacity=cap, **kws[0])
    _equal(tuple(c[:cap] for c in cut[:4]) + (cut[4],), tuple(g[:cap] for g in got[0][:4]) + (got[0][4],), "capacity")
    eng.check_status()


def test_f16_range_is_the_calls(eng, sd):
    """One row far outside the f16 range in the last block only: every block takes the datapath score_all_pairs takes on
    the whole rectangle (test_gpu_seq_above.test_f16_range_is_the_calls' construction)."""
    m, L = M_A, 8
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
    cut = _quantile(eng, score, L, 0.001)
    rt, ct = _tab([rb], r), _tab([m // 2], m)
    got = _pooled_equals_resident(eng, rows, cols, L, cut, (
        dict(row_sessions=rt, col_sessions=ct, min_terms=4, window=-1, context=L - 1),
        dict(col_sessions=ct, min_terms=2, window=5, row0=5, causal=True, reverse=True)), "mixed range", score=score)
    assert all(g[0].numel() > 0 for g in got)
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 3. the Python surface
def test_loop_closures_above_sessions(model):
    e = model.engine()
    pooled = _pooled(150, 32, 3.0, 78)
    starts = [0, 60, 100]
    thr = _quantile(e, e.score_all_pairs(pooled, pooled), 8, 0.05)
    # the four new arguments at their defaults: today's calls and tuples
    _equal(model.loop_closures_above(pooled, pooled, thr, window=16, seq_slopes=None, row_sessions=None, col_sessions=None,
                                     min_terms=1), e.score_above(pooled, pooled, thr, window=16), "defaults, L = 1")
    _equal(model.loop_closures_above(pooled, pooled, thr, window=16, seq_len=8),
           e.score_seq_above(pooled, pooled, 8, thr, window=16), "defaults, L = 8")
    want = e.score_session_above(pooled, pooled, 8, thr, row_sessions=starts, col_sessions=starts, min_terms=4, window=16)
    assert want[0].numel() > 0
    _equal(model.loop_closures_above(pooled, pooled, thr, window=16, seq_len=8, row_sessions=starts, col_sessions=starts,
                                     min_terms=4), want, "tables, min_terms")
    paths = seq_path_ref.seq_paths(8, ["1", "1/2", "2"])
    _equal(model.loop_closures_above(pooled, pooled, thr, window=16, seq_len=8, seq_slopes=["1", "1/2", "2"], causal=True,
                                     col_sessions=starts, seq_reverse=True, capacity=50),
           e.score_session_above(pooled, pooled, 8, thr, paths, col_sessions=starts, window=16, causal=True, reverse=True,
                                 capacity=50), "slopes, capacity")
    _equal(model.loop_closures_above(pooled, pooled, thr, window=16, seq_len=8, min_terms=8),
           e.score_session_above(pooled, pooled, 8, thr, min_terms=8, window=16), "min_terms alone")
    e.check_status()


def test_place_database_online_equals_offline(model):
    """query_closures before every append (causal, L = 8, min_terms = 3), new_session() called twice on the way, against
    one query_ids_closures call over the whole map; window >= the paths' largest offset, so no reverse sum of an eligible
    column of the current session reaches a member that is not stored yet."""
    from sg_pr_amd import engine
    from sg_pr_amd.place_db import PlaceDatabase
    n, L, mt = 120, 8, 3
    seams = (50, 53)                                           # the third session starts three scans into the second
    paths = engine.seq_paths(L, seq_path_ref.SLOPES)
    window = int(paths.max())
    pooled = _pooled(n, 32, 3.0, 77)
    e = model.engine()
    thr = _quantile(e, e.score_all_pairs(pooled, pooled), L, 0.2)
    for slopes, table in ((seq_path_ref.SLOPES, paths), (None, None)):
        db = PlaceDatabase(model, capacity=4)
        got = []
        for t in range(n):
            if t in seams:
                db.new_session()
            rows, ids, vals, codes, row_ptr = db.query_closures(None, None, thr, seq_len=L, slopes=slopes, min_terms=mt,
                                                                window=window, causal=True, pooled=pooled[t:t + 1])
            assert row_ptr.tolist() == [0, rows.numel()] and not rows.any()
            got.append((rows + t, ids, vals, codes))
            db.append_pooled(pooled[t:t + 1])
        starts = db.session_starts
        assert starts.tolist() == [0, 50, 53]
        online = tuple(torch.cat([g[j] for g in got]) for j in range(4))
        offline = db.query_ids_closures(0, n, thr, seq_len=L, slopes=slopes, min_terms=mt, window=window, causal=True)
        _equal(offline, e.score_session_above(pooled, pooled, L, thr, table, row_sessions=starts, col_sessions=starts,
                                              min_terms=mt, window=window, causal=True), ("offline", slopes))
        assert offline[0].numel() > 50
        _equal(online, offline[:4], ("online / offline", slopes))
        counts = torch.tensor([g[0].numel() for g in got])
        assert torch.equal(torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0))), offline[4].cpu())
        # rows 50, 51 and 53, 54 have fewer than three terms: never listed
        assert not np.isin(offline[0].cpu().numpy(), (0, 1, 50, 51, 53, 54)).any()
        # a run of members across both seams
        want = db.query_ids_closures(0, n, thr, seq_len=L, slopes=slopes, min_terms=mt, window=window)
        run = db.query_ids_closures(40, 30, thr, seq_len=L, slopes=slopes, min_terms=mt, window=window)
        lo, hi = int(want[4][40]), int(want[4][70])
        _equal(run[:4], (want[0][lo:hi] - 40,) + tuple(w[lo:hi] for w in want[1:4]), ("a run", slopes))
        assert torch.equal(run[4], want[4][40:71] - lo)
    for bad in (lambda: db.query_ids_above([0], 0.5), lambda: db.query_ids_seq_above(0, 3, L, 0.5)):
        with pytest.raises(NotImplementedError, match="query_closures"):
            bad()
    # one session: the lists of the one-trajectory call
    one = PlaceDatabase(model, capacity=4)
    one.append_pooled(pooled)
    _equal(one.query_ids_closures(40, 30, thr, seq_len=L, window=window),
           one.query_ids_seq_above(40, 30, L, thr, window=window), "one session")
    e.check_status()


def test_place_db_cli_session_above(model, tmp_path, ckpt_path, capsys):
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
    eng = model.engine()
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    base = [str(cfg), "--window", "14", "--threshold", "0.9"]
    place_db.main(base + ["--seq-len", "8"])                  # without sessions or slopes: as before, no new file
    assert not os.path.exists(eva / "07_session_above.npz")
    plain = {k: v.copy() for k, v in np.load(eva / "07_seq_above.npz").items()}
    capsys.readouterr()
    nine = seq_path_ref.seq_paths(8, ["1", "1/2", "2"])
    for extra, starts, paths, mt in ((["--sessions", "3", "--seq-len", "8", "--min-terms", "4"], [0, 40, 80], None, 4),
                                     (["--seq-len", "8", "--seq-slopes", "1,1/2,2"], [0], nine, 1),
                                     (["--sessions", "3", "--seq-len", "8", "--seq-slopes", "1,1/2,2", "--min-terms", "2"],
                                      [0, 40, 80], nine, 2)):
        place_db.main(base + extra)
        out = capsys.readouterr().out
        again = np.load(eva / "07_seq_above.npz")            # everything it wrote before, byte for byte
        for k in plain:
            assert again[k].tobytes() == plain[k].tobytes(), k
        z = np.load(eva / "07_session_above.npz")
        assert sorted(z.files) == ["codes", "cols", "min_terms", "precision", "recall", "row_ptr", "rows", "scores", "seq_len",
                                   "session_starts"]
        assert z["session_starts"].tolist() == starts and int(z["min_terms"]) == mt and int(z["seq_len"]) == 8
        rows, cols, vals, codes, row_ptr = eng.score_session_above(pooled, pooled, 8, 0.9, paths, row_sessions=starts,
                                                                   col_sessions=starts, min_terms=mt, window=14)
        assert rows.numel() > 0
        assert np.array_equal(z["rows"], rows.cpu().numpy()) and np.array_equal(z["cols"], cols.cpu().numpy())
        assert np.array_equal(z["scores"].view(np.uint32), vals.cpu().numpy().view(np.uint32))
        assert np.array_equal(z["codes"], codes.cpu().numpy()) and np.array_equal(z["row_ptr"], row_ptr.cpu().numpy())
        line = [l for l in out.splitlines() if " min terms %d " % mt in l]
        assert len(line) == 1 and "pairs %d" % rows.numel() in line[0], out
        assert "precision %.4f recall %.4f" % (float(z["precision"]), float(z["recall"])) in line[0]
        assert 0.0 <= float(z["precision"]) <= 1.0 and 0.0 <= float(z["recall"]) <= 1.0
    for bad in (["--min-terms", "2"], ["--threshold", "0.9", "--seq-len", "8", "--min-terms", "9"],
                ["--threshold", "0.9", "--min-terms", "0"]):
        with pytest.raises(SystemExit):
            place_db.main([str(cfg)] + bad)
    eng.check_status()


def test_session_above_bench_tool(capsys):
    import json
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import session_above_bench
    recs = session_above_bench.main(["--small"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert lines == recs and len(recs) == 16
    assert {(r["shape"], r["seq_len"], r["sessions"], r["paths"], r["min_terms"]) for r in recs} == \
        {(s, L, n, p, mt) for s in ("square", "one query") for L in (8, 32)
         for n, p, mt in ((1, "unit", 1), (4, "unit", 1), (4, "unit", L // 2), (4, "nine", L // 2))}
    assert all(r["equal_resident"] and r["fused_ms"] > 0 and r["fused_peak_mb"] >= 0 for r in recs)
    assert all(r["equal_matrix"] and r["matrix_ms"] > 0 for r in recs if r["min_terms"] == 1)
    assert all(r["equal_seq"] and r["seq_ms"] > 0 and r["fused_over_seq"] > 0 for r in recs if r["sessions"] == 1)
    assert sum(r["pairs"] > 0 for r in recs) >= 8
