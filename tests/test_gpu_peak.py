"""sgpr_peak_filter / sgpr_score_peak_topk on the GPU, every comparison bit for bit against the NumPy reference
(tests/peak_ref.py): the filter on synthetic matrices at every strip edge and tie case, the pooled form against
score_all_pairs of the whole rectangle -> seq_ref -> peak_ref -> the list reference (one block and several, on every kind
of handle, dirty workspaces), the place database online against one offline call, two streams, NaN graphs, and the
Python surface (SG.loop_closures, the place_db CLI, tools/peak_bench.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import peak_ref
import seq_ref
from test_gpu_row_blocks import M_A, RB_A
from test_gpu_score_range import _any_shape, _wide_checkpoint
from test_gpu_seq import _flags, _pooled, _seq_rb
from test_gpu_stateless import _Poison, _dptr, _ff

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 1024                          # peak_filter_kernel's strip (sgpr_peak.hip, SGPR_PEAK_STRIP): columns per workgroup
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def sd(ckpt_path):
    from oracle import sgpr_oracle
    return sgpr_oracle.load_checkpoint(ckpt_path)


@pytest.fixture(scope="module")
def eng(sd):
    from sg_pr_amd import engine
    e = engine.Engine(sd, device=0)
    assert e.PEAK_STRIP == S
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


def _bits_equal(got, want, what):
    """float32 arrays without NaN on the reference's side: the same bit pattern everywhere"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _lists_equal(got, want, what):
    """(values, indices[, dirs]) device tensors against host arrays"""
    assert len(got) == len(want), what
    _bits_equal(got[0].cpu().numpy(), want[0], (what, "values"))
    for j in range(1, len(want)):
        g = got[j].cpu().numpy()
        assert g.shape == want[j].shape and g.dtype == want[j].dtype, (what, j, g.shape, g.dtype)
        bad = g != want[j]
        assert not bad.any(), (what, "output", j, int(bad.sum()), np.argwhere(bad)[:5].tolist())


# ------------------------------------------------------------------------------------------------- 1. the filter
def _matrix(r, m, ld, rho, seed):
    """values quantised to 4 levels (ties straddle every strip boundary) with NaN, +-inf and -0.0 / +0.0 sprinkled in;
    with 5 rows: row 1 constant, row 2 a plateau of the row's largest value longer than rho, row 3 all NaN, row 4 a
    would-be peak every 9 columns with a NaN on either side and -0.0 beside +0.0 in between -> host float32 [r, ld]"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 4, size=(r, ld)) / np.float32(4.0)).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    for val, frac in ((np.nan, 0.03), (np.inf, 0.004), (-np.inf, 0.02), (-0.0, 0.03), (0.0, 0.03)):
        flat[rng.integers(0, n, size=max(1, int(n * frac)))] = val
    if r >= 5:
        x[1] = 0.5
        x[2][x[2] == np.inf] = 0.25                                  # (the plateau is the row's largest value)
        x[2, m // 3:m // 3 + min(rho, m) + 3] = 2.0
        x[3] = np.nan
        x[4] = np.where(np.arange(ld) % 2 == 0, np.float32(-0.0), np.float32(0.0))
        x[4, 4::9] = 1.0
        x[4, 3::9] = np.nan
        x[4, 5::9] = np.nan
    return x


def _modes(r, m):
    table = np.array([0, m - 1, m // 2, 3, m // 3], dtype=np.int32)[:r]
    return [dict(window=-1), dict(window=0), dict(window=50, row0=3), dict(window=50, causal=True, row0=m // 2),
            dict(window=-1, causal=True, row0=0),                    # row 0 has no eligible column
            dict(window=7, causal=True, row_self=table),             # ... and so has the table's first row
            dict(window=0, row_self=table)]


@pytest.mark.parametrize("rho", [0, 1, 7, 1024])
def test_filter_equals_the_reference(eng, rho):
    sizes = sorted({1, 2, rho, rho + 1, S - 1, S, S + 1, 2 * S + rho + 3, 3000} - {0})
    peaks = 0
    for m in sizes:
        for r in (1, 5):
            ld, ldo = m + 5, m + 8                                   # ld > M and ldo > ld
            host = _matrix(r, m, ld, rho, 13 * m + r + rho)
            dev = torch.from_numpy(host).cuda()
            for j, mode in enumerate(_modes(r, m)):
                want = peak_ref.peak_filter(host[:, :m], rho, **mode)
                out = torch.full((r, ldo), 7.0, device="cuda")
                kw = dict(mode)
                if "row_self" in kw:
                    kw["row_self"] = torch.from_numpy(kw["row_self"])
                got = eng.peak_filter(dev[:, :m], rho, out=out[:, :m], **kw)
                what = (rho, m, r, mode)
                assert got.data_ptr() == out.data_ptr()
                full = out.cpu().numpy()
                _bits_equal(np.ascontiguousarray(full[:, :m]), want, what)    # every entry of [R][M] is written ...
                assert (full[:, m:] == 7.0).all(), what                       # ... and nothing beyond M
                peaks += int((want != -INF).sum())
                if j == 0 and r == 5:                                         # (every column eligible)
                    assert (want[3] == -INF).all()                            # an all-NaN row
                    if rho <= 8:                                              # NaN neighbours suppress nothing
                        assert (want[4, np.arange(4, m, 9)] == 1.0).all(), what
                    first = [0] if rho >= 1 else list(range(m))               # a constant row: its first column
                    assert np.flatnonzero(want[1] != -INF).tolist() == first, what
                    if rho >= 1:                                              # a plateau longer than rho: its first column
                        lo = m // 3
                        assert want[2, lo] == 2.0 and (want[2, lo + 1:lo + min(rho, m) + 3] == -INF).all(), what
            # contiguous, no `out`: the allocation path
            _bits_equal(eng.peak_filter(torch.from_numpy(np.ascontiguousarray(host[:, :m])).cuda(), rho).cpu().numpy(),
                        peak_ref.peak_filter(host[:, :m], rho), (rho, m, r, "contiguous"))
    assert peaks > 0
    assert eng.peak_filter(torch.zeros(0, 7).cuda(), rho).shape == (0, 7)
    assert eng.peak_filter(torch.zeros(3, 0).cuda(), rho).shape == (3, 0)


def test_filter_tie_cases_by_hand(eng):
    """the reference's by-hand cases (tests/test_peak_host.py) on the device, at both sides of a strip boundary"""
    for m, at in ((40, 0), (2 * S + 40, S - 4), (2 * S + 40, 2 * S - 15)):
        x = np.full((1, m), -1.0, dtype=np.float32)
        x[0, at:at + 9] = [0.5, 0.5, 0.25, np.nan, 0.5, 0.0, -0.0, -np.inf, np.inf]
        for rho, want in ((1, [0, 4, 8]), (2, [0, 4, 8]), (3, [0, 8]), (4, [0, 8])):
            p = eng.peak_filter(x, rho).cpu().numpy()
            _bits_equal(p, peak_ref.peak_filter(x, rho), (m, at, rho))
            near = np.flatnonzero(p[0, at:at + 9] != -INF).tolist()
            assert near == want, (m, at, rho, near)
        flat = np.full((1, m), 0.5, dtype=np.float32)                 # a plateau longer than rho: its first column
        assert np.flatnonzero(eng.peak_filter(flat, 4).cpu().numpy()[0] != -INF).tolist() == [0]
        got = np.flatnonzero(eng.peak_filter(flat, 4, window=2, row0=at + 10).cpu().numpy()[0] != -INF).tolist()
        assert got == [0, at + 13], (m, at, got)
    from sg_pr_amd.engine import SgprError
    with pytest.raises(SgprError, match="radius"):
        eng.peak_filter(np.zeros((2, 5), dtype=np.float32), 1025)


# ------------------------------------------------------------------------------------------------- 2. one block
@pytest.fixture(scope="module")
def world(eng):
    """the shipped checkpoint on synth.world_sequence(160, 100, seed=0): pooled vectors and score_all_pairs of the
    whole rectangle - the yardstick - on the host"""
    from sg_pr_amd import synth
    centers, labels, _, _ = synth.world_sequence(160, 100, seed=0)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    return pooled, eng.score_all_pairs(pooled, pooled).cpu().numpy()


def _reference(score, L, rho, k, reverse, ctx=0, **elig):
    """host: seq_ref -> peak_ref -> the list reference; dirs gathered at the listed columns, 0 in a padding slot"""
    q, d = seq_ref.seq_filter(score, L, ctx, **_flags(reverse))
    elig = dict(elig)
    elig["row0"] = elig.get("row0", 0) + ctx
    if elig.get("row_self") is not None:
        elig["row_self"] = np.asarray(elig["row_self"])[ctx:]
    v, i = peak_ref.peak_lists(q, rho, k, **elig)
    dirs = np.where(i >= 0, np.take_along_axis(d, np.maximum(i, 0).astype(np.int64), axis=1), 0).astype(np.uint8)
    return v, i, dirs


@pytest.mark.parametrize("L", [1, 8])
def test_pooled_equals_matrix_reference(eng, world, L):
    pooled, score = world
    r = m = 160
    distinct_somewhere = False
    for reverse in (False, True, "both"):
        for ctx in (0, 7):
            for mode in (dict(window=-1), dict(window=16, causal=True)):
                for rho in (0, 5, 60):
                    for k in (1, 4, 40):
                        what = (L, reverse, ctx, mode, rho, k)
                        got = eng.score_peak_topk(pooled, pooled, rho, seq_len=L, k=k, context=ctx, reverse=reverse, **mode)
                        want = _reference(score, L, rho, k, reverse, ctx=ctx, **mode)
                        assert got[0].shape == (r - ctx, k)
                        _lists_equal(got, want, what)
                        if rho == 0:                          # the bits of sgpr_score_seq_topk, on the device as well
                            plain = eng.score_seq_topk(pooled, pooled, L, k=k, context=ctx, reverse=reverse, **mode)
                            _lists_equal(got, tuple(t.cpu().numpy() for t in plain), (what, "score_seq_topk"))
                        elif k == 4:
                            plain = eng.score_seq_topk(pooled, pooled, L, k=k, context=ctx, reverse=reverse, **mode)[1]
                            distinct_somewhere |= bool((plain != got[1]).any())
                            for row in want[1]:                               # peaks are more than rho apart
                                assert (np.diff(np.sort(row[row >= 0])) > rho).all(), what
    assert distinct_somewhere
    # row_self, row0 > 0, k beyond M
    perm = np.random.default_rng(3).permutation(m).astype(np.int32)
    for kw in (dict(window=10, row_self=perm), dict(window=10, causal=True, row_self=perm), dict(window=20, row0=37),
               dict(window=0, row0=37, causal=True)):
        dev_kw = {a: (torch.from_numpy(b) if a == "row_self" else b) for a, b in kw.items()}
        got = eng.score_peak_topk(pooled, pooled, 5, seq_len=L, k=m + 5, context=3, reverse="both", **dev_kw)
        _lists_equal(got, _reference(score, L, 5, m + 5, "both", ctx=3, **kw), (L, kw))
    # context == R: empty lists; no columns: padding only
    v, i, d = eng.score_peak_topk(pooled, pooled, 5, seq_len=L, k=3, context=r)
    assert v.shape == (0, 3) and i.shape == (0, 3) and d.shape == (0, 3)
    v, i, d = eng.score_peak_topk(pooled, pooled[:0], 5, seq_len=L, k=3, context=2, reverse=True)
    assert v.shape == (r - 2, 3) and (v == -float("inf")).all() and (i == -1).all() and not d.any()
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 3. several blocks
def _several_blocks(e, width, scale, cases, what):
    """the lists of a call that runs more than one 64 MB block against the one-rectangle reference, twice on one arena
    of random bytes: the second call finds the workspace the first one left"""
    m, r = M_A, RB_A + 1
    rows, cols = _pooled(r, width, scale, r), _pooled(m, width, scale, m)
    score = e.score_all_pairs(rows, cols).cpu().numpy()
    for L, rho, kw in cases:
        assert _seq_rb(r, m, L) < r                                  # more than one block runs
        reverse, ctx = kw.get("reverse", False), kw.get("context", 0)
        need = e.score_peak_topk_workspace_bytes(r, m, rho, seq_len=L, k=kw["k"], causal=kw.get("causal", False),
                                                 context=ctx, reverse=reverse)
        assert need < 4.2 * (64 << 20) + 64 * m                      # score, P, Q and dir blocks; never R x M
        elig = {a: b for a, b in kw.items() if a in ("window", "row0", "causal")}
        want = _reference(score, L, rho, kw["k"], reverse, ctx=ctx, **elig)
        with _Poison(e, "arena", seed=5, arena_bytes=need):
            first = e.score_peak_topk(rows, cols, rho, seq_len=L, **kw)
            again = e.score_peak_topk(rows, cols, rho, seq_len=L, **kw)
            torch.cuda.synchronize()
        _lists_equal(first, want, (what, L, rho, kw))
        _lists_equal(again, want, (what, L, rho, kw, "dirtied workspace"))
    e.check_status()


def test_several_blocks_tuned_handle(eng):
    _several_blocks(eng, 32, 3.0, [(8, 5, dict(k=17, window=50, context=7, reverse="both")),
                                   (1, 60, dict(k=4, window=5, row0=7, causal=True))], "tuned")


def test_several_blocks_wide_checkpoint(sd):
    from sg_pr_amd import engine
    wide = engine.Engine(_wide_checkpoint(sd), device=0)
    try:
        assert not wide.uses_f16_planes()
        _several_blocks(wide, 32, 3.0, [(8, 5, dict(k=17, window=50, context=7, reverse="both"))], "wide checkpoint")
    finally:
        wide.close()


def test_several_blocks_any_shape():
    any_eng = _any_shape(_any_shape())
    try:
        assert any_eng.any_shape
        _several_blocks(any_eng, 48, 1.0, [(8, 5, dict(k=17, window=50, causal=True, context=2, reverse=True))], "any-shape")
    finally:
        any_eng.close()


# ------------------------------------------------------------------------------------------------- 4. online = offline
def test_place_database_online_equals_offline(model):
    """40 scans added one at a time, each queried first (causal, distinct=5, k=3) with seq_len 1 and 4 (window 3 >=
    seq_len - 1): a column that is not in the database yet does not qualify, so it cannot suppress - the lists are
    those of one offline causal call."""
    from sg_pr_amd import synth
    from sg_pr_amd.place_db import PlaceDatabase
    n, k, rho, window = 40, 3, 5, 3
    centers, labels, _, _ = synth.world_sequence(n, 100, seed=1)
    db = PlaceDatabase(model, capacity=4)
    one, four = [], []
    for t in range(n):
        c, l = centers[t:t + 1], labels[t:t + 1]
        one.append(db.query(c, l, k=k, window=window, causal=True, distinct=rho))
        four.append(db.query_seq(c, l, 4, k=k, window=window, causal=True, distinct=rho))
        db.add(c, l)
    e = model.engine()
    pooled = db.pooled
    off1 = e.score_peak_topk(pooled, pooled, rho, seq_len=1, k=k, window=window, causal=True)
    off4 = e.score_peak_topk(pooled, pooled, rho, seq_len=4, k=k, window=window, causal=True, reverse="both")
    _lists_equal(tuple(torch.cat([g[j] for g in one]) for j in range(2)), tuple(t.cpu().numpy() for t in off1[:2]), "L = 1")
    _lists_equal(tuple(torch.cat([g[j] for g in four]) for j in range(3)), tuple(t.cpu().numpy() for t in off4), "L = 4")
    assert (off1[1][:window + 1] == -1).all() and (off1[1][n - 1] >= 0).any()
    # ... and both are the reference's lists of the offline matrix
    score = e.score_all_pairs(pooled, pooled).cpu().numpy()
    _lists_equal(off1[:2], _reference(score, 1, rho, k, False, window=window, causal=True)[:2], "offline, L = 1")
    _lists_equal(off4, _reference(score, 4, rho, k, "both", window=window, causal=True), "offline, L = 4")
    # members: query_ids / query_ids_seq
    ids = torch.tensor([39, 5, 20, 33])
    got = db.query_ids(ids, k=k, window=window, distinct=rho)
    want = peak_ref.peak_lists(score[ids.numpy()], rho, k, window=window, row_self=ids.numpy())
    _lists_equal(got, want, "query_ids")
    run = db.query_ids_seq(10, 25, 4, k=k, window=window, distinct=rho)
    full = _reference(score, 4, rho, k, "both", window=window)
    _lists_equal(run, tuple(w[10:35] for w in full), "query_ids_seq")
    e.check_status()


# ------------------------------------------------------------------------------------------------- 5. two streams
def test_two_streams_write_prefilled_outputs(eng):
    lib, h = eng.lib, eng._h
    rows_a, cols_a = _pooled(300, 32, 3.0, 31), _pooled(1200, 32, 3.0, 32)
    rows_b, cols_b = _pooled(250, 32, 3.0, 33), _pooled(2100, 32, 3.0, 34)
    block = eng.score_all_pairs(rows_b, cols_b)
    ka, kb = 8, 3
    want_a = eng.score_peak_topk(rows_a, cols_a, 10, seq_len=8, k=ka, window=20, context=7, reverse="both")
    want_b = eng.score_peak_topk(rows_b, cols_b, 50, seq_len=1, k=kb, window=5, causal=True, row0=900)
    want_p = eng.peak_filter(block, 50, window=5, causal=True, row0=900)
    na = eng.score_peak_topk_workspace_bytes(300, 1200, 10, seq_len=8, k=ka, context=7, reverse="both")
    nb = eng.score_peak_topk_workspace_bytes(250, 2100, 50, seq_len=1, k=kb, causal=True)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        va, ia, da = _ff(293 * ka, torch.float32), _ff(293 * ka, torch.int32), _ff(293 * ka, torch.uint8)
        vb, ib = _ff(250 * kb, torch.float32), _ff(250 * kb, torch.int32)
        pb = _ff(250 * 2100, torch.float32)
        wsa, wsb = _ff(na, torch.uint8), _ff(nb, torch.uint8)
        torch.cuda.synchronize()
        rc_a = lib.sgpr_score_peak_topk(h, _dptr(rows_a), 300, _dptr(cols_a), 1200, 7, None, 0, 20, 2 | 4, 8, 10, ka,
                                        _dptr(va), _dptr(ia), _dptr(da), _dptr(wsa), na, ctypes.c_void_p(sa.cuda_stream))
        rc_b = lib.sgpr_score_peak_topk(h, _dptr(rows_b), 250, _dptr(cols_b), 2100, 0, None, 900, 5, 1 | 2, 1, 50, kb,
                                        _dptr(vb), _dptr(ib), None, _dptr(wsb), nb, ctypes.c_void_p(sb.cuda_stream))
        rc_p = lib.sgpr_peak_filter(h, _dptr(block), 250, 2100, 2100, None, 900, 5, 1, 50, _dptr(pb), 2100,
                                    ctypes.c_void_p(sb.cuda_stream))
        torch.cuda.synchronize()
        assert (rc_a, rc_b, rc_p) == (0, 0, 0), lib.sgpr_last_error()
        _lists_equal((va.view(293, ka), ia.view(293, ka), da.view(293, ka)), tuple(t.cpu().numpy() for t in want_a), "stream a")
        _lists_equal((vb.view(250, kb), ib.view(250, kb)), tuple(t.cpu().numpy() for t in want_b[:2]), "stream b")
        _bits_equal(pb.view(250, 2100).cpu().numpy(), want_p.cpu().numpy(), "stream b, filter")
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 6. NaN graphs
def test_nan_graphs(eng, world):
    pooled, _ = world
    rows, cols = pooled.clone(), pooled.clone()
    rows[5, 3] = float("nan")
    cols[20, 0] = float("nan")
    score = eng.score_all_pairs(rows, cols).cpu().numpy()
    assert np.isnan(score[5]).all() and np.isnan(score[:, 20]).all()
    for L, reverse in ((1, False), (4, "both")):
        for rho in (0, 5, 60):
            got = eng.score_peak_topk(rows, cols, rho, seq_len=L, k=6, window=-1, reverse=reverse)
            _lists_equal(got, _reference(score, L, rho, 6, reverse), ("NaN graphs", L, rho))
            v, i = got[0].cpu().numpy(), got[1].cpu().numpy()
            assert (i[5] == -1).all() and (v[5] == -INF).all()        # a NaN row graph: padding lists
            assert not (i == 20).any()                                # a NaN column graph is never listed ...
            if L == 1:
                # ... and never suppresses: the lists are those of the matrix without that column's values
                gone = np.where(np.isnan(score), -INF, score)
                _lists_equal(got[:2], peak_ref.peak_lists(gone, rho, 6), ("NaN column as -inf", rho))
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 7. the Python surface
def test_loop_closures_distinct(model, world):
    pooled, score = world
    for kw in (dict(k=4, window=16), dict(k=4, window=16, seq_len=8), dict(k=2, window=16, causal=True, seq_len=8, seq_reverse=False)):
        base = model.loop_closures(pooled, pooled, **kw)
        same = model.loop_closures(pooled, pooled, distinct=None, **kw)      # the default: today's path and results
        assert len(base) == len(same) == (3 if kw.get("seq_len", 1) > 1 else 2)
        for b, s in zip(base, same):
            assert b.dtype == s.dtype and torch.equal(b.view(torch.int32) if b.dtype == torch.float32 else b,
                                                      s.view(torch.int32) if s.dtype == torch.float32 else s)
        got = model.loop_closures(pooled, pooled, distinct=10, **kw)
        L = kw.get("seq_len", 1)
        elig = dict(window=16, causal=kw.get("causal", False))
        want = _reference(score, L, 10, kw["k"], kw.get("seq_reverse", "both") if L > 1 else False, **elig)
        assert len(got) == len(base)
        _lists_equal(got, want[:len(got)], ("loop_closures", kw))
        zero = model.loop_closures(pooled, pooled, distinct=0, **kw)         # rho = 0: the plain lists
        assert torch.equal(zero[1], base[1]) and torch.equal(zero[0].view(torch.int32), base[0].view(torch.int32))


def test_place_db_cli_distinct(model, tmp_path, ckpt_path, capsys):
    from sg_pr_amd import graph_store, metrics, place_db, synth
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
    eng = model.engine()
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    for extra, L in (([], 1), (["--seq-len", "8"], 8)):
        place_db.main([str(cfg), "--k", "3", "--window", "10", "--distinct", "5"] + extra)
        line = next(l for l in capsys.readouterr().out.splitlines() if "distinct radius" in l)
        assert "recall@1" in line and "recall@3" in line and "places per list" in line, line
        z = np.load(tmp_path / "eva" / "07_distinct.npz")
        assert int(z["radius"]) == 5 and z["indices"].shape == z["scores"].shape == (n, 3) and z["recall"].shape == (3,)
        v, i, d = eng.score_peak_topk(pooled, pooled, 5, seq_len=L, k=3, window=10, reverse="both" if L > 1 else False)
        assert np.array_equal(z["indices"], i.cpu().numpy())
        assert np.array_equal(z["scores"].view(np.uint32), v.cpu().numpy().view(np.uint32))
        assert ("dirs" in z.files) == (L > 1) and (L == 1 or np.array_equal(z["dirs"], d.cpu().numpy()))
        plain = np.load(tmp_path / "eva" / "07_topk.npz")["indices"]            # the plain lists are still written
        assert metrics.places_per_list(z["indices"], 5) >= metrics.places_per_list(plain, 5) >= 1.0
        assert "%.3f (plain %.3f)" % (metrics.places_per_list(z["indices"], 5), metrics.places_per_list(plain, 5)) in line
        assert metrics.places_per_list(z["indices"], 5) == peak_ref.places_per_list(z["indices"], 5)
    place_db.main([str(cfg), "--k", "3", "--window", "10", "--distinct", "5", "--verify"])
    line = next(l for l in capsys.readouterr().out.splitlines() if "pairs verified" in l)
    plain = np.load(tmp_path / "eva" / "07_topk.npz")["indices"]
    dz = np.load(tmp_path / "eva" / "07_distinct_verify.npz")
    assert "plain %d distinct %d" % (int((plain >= 0).sum()), int(dz["verified"])) in line, line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--distinct", "1025"])


def test_peak_bench_tool(capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import peak_bench
    recs = peak_bench.main(["--tiny"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert lines == recs
    calls = [r for r in recs if "peak_ms" in r]
    assert {(r["shape"], r["seq_len"], r["k"], r["radius"]) for r in calls} == {
        (s, L, k, rho) for s in ("square", "one query") for L in (1, 8) for k in (4, 16) for rho in (0, 10, 50, 1024)}
    assert all(r["peak_ms"] > 0 and r["plain_ms"] > 0 and r["peak_over_plain"] > 0 for r in calls)
    square = [r for r in calls if r["shape"] == "square"]
    assert all(r["places_per_list"] >= r["places_per_list_plain"] >= 1.0 for r in square if r["radius"] > 0)
    filt = [r for r in recs if "filter_ms" in r]
    assert len(filt) == 8 and all(r["filter_ms"] > 0 and r["copy_ms"] > 0 for r in filt)
