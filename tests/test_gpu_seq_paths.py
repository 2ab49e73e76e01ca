"""sgpr_seq_path_filter / sgpr_score_path_topk on the GPU: the path filter against the NumPy reference bit for bit, the
unit path against sgpr_seq_filter / sgpr_score_seq_topk / sgpr_score_peak_topk, the pooled form against score_all_pairs
-> seq_path_filter -> (peak_filter ->) topk_rows_large on the same rectangle (one block and several, on every kind of
handle), dirty workspaces, pre-filled outputs on two streams, the planted revisits of another slope, the place database
online against one offline call, and the Python surface (SG.loop_closures, the place_db CLI, tools/path_bench.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import seq_path_ref
import seq_ref
from test_gpu_row_blocks import M_A, RB_A
from test_gpu_score_range import _any_shape, _wide_checkpoint
from test_gpu_seq import DIRECTIONS, LENGTHS, _equal, _flags, _pooled, _same_bits, _scores, _seq_rb
from test_gpu_stateless import _check_all_patterns, _dptr, _ff
from test_seq_paths_host import PLANTED_SLOPES, planted_figures

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TR, TC = 32, 256                  # seq_path_kernel's tile (SEQ_TR, SEQ_TC of sgpr_seq.hip): output rows x columns


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


def _path_sets(L):
    """(name, table): the unit path; the 9-path set; the all-zero path plus one whose only step is a jump of 64 at
    d = L - 1 (both halos used to the last word); 16 copies of one path"""
    jump = np.zeros((2, L), dtype=np.int32)
    if L > 1:
        jump[1, L - 1] = 64
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    return [("unit", seq_path_ref.unit_path(L)), ("nine", nine), ("jump", jump),
            ("copies", np.repeat(nine[-1:], 16, axis=0))]


# ------------------------------------------------------------------------------------------------- 1. the filter
FILTER_SHAPES = [(1, 1, 0, 0), (5, 7, 0, 0), (37, 131, 0, 0), (70, 300, 3, 5),
                 (TR + 1, TC - 1, 0, 0), (TR + 1, TC + 1, 0, 0), (TR + 1, 2 * TC + 3, 0, 0)]


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=["%dx%d" % s[:2] for s in FILTER_SHAPES])
def test_filter_equals_the_reference(eng, shape):
    r, m, pad_in, pad_out = shape
    host = _scores(r, m, 7 * r + m, ld=m + pad_in)
    dev = torch.from_numpy(host).cuda()[:, :m]               # ld = m + pad_in: read in place
    assert dev.stride(0) == m + pad_in or r == 1
    winners = set()
    for L in LENGTHS:
        for name, paths in _path_sets(L):
            for reverse in DIRECTIONS:
                wq, wc = seq_path_ref.path_filter(host[:, :m], paths, 0, **_flags(reverse))
                winners.update(np.unique(wc).tolist())
                for ctx in sorted({0, min(1, r), min(L - 1, r), r - 1}):
                    ro = r - ctx
                    out = torch.full((ro, m + pad_out), 7.0, device="cuda")
                    ocode = torch.full((ro, m + pad_out), 99, dtype=torch.uint8, device="cuda")
                    q, c = eng.seq_path_filter(dev, L, paths, context=ctx, reverse=reverse, out=out[:, :m],
                                               out_code=ocode[:, :m])
                    what = (shape, L, name, reverse, ctx)
                    _same_bits(q.cpu().numpy(), wq[ctx:], what)
                    assert np.array_equal(c.cpu().numpy(), wc[ctx:]), what
                    if pad_out:                               # nothing written past column m of an output row
                        assert (out[:, m:] == 7.0).all() and (ocode[:, m:] == 99).all(), what
                if name == "nine":
                    q2 = eng.seq_path_filter(dev, L, paths, reverse=reverse)      # without the code
                    _same_bits(q2.cpu().numpy(), wq, (shape, L, name, reverse, "no code"))
    if r > 30:
        assert len(winners) >= 12                             # many paths win somewhere, in both directions
    assert eng.seq_path_filter(dev, 3, seq_path_ref.unit_path(3), context=r).shape == (0, m)


# ------------------------------------------------------------------------------------------------- 2. the unit path
def test_unit_path_filter_is_seq_filter(eng):
    dev = torch.from_numpy(_scores(70, 300, 5)).cuda()
    for L in LENGTHS:
        for reverse in DIRECTIONS:
            for ctx in (0, L - 1):
                want = eng.seq_filter(dev, L, context=ctx, reverse=reverse, want_dir=True)
                got = eng.seq_path_filter(dev, L, seq_path_ref.unit_path(L), context=ctx, reverse=reverse, want_code=True)
                _equal(got, want, ("unit path", L, reverse, ctx))


def test_unit_path_pooled_is_seq_topk_and_peak_topk(eng):
    rows, cols = _pooled(300, 32, 3.0, 1), _pooled(517, 32, 3.0, 2)
    n = 0
    for L in (1, 8, 32):
        unit = seq_path_ref.unit_path(L)
        for k in (1, 17):
            for elig in (dict(window=-1), dict(window=50, causal=True), dict(window=10, row0=3)):
                reverse = DIRECTIONS[n % 3]
                n += 1
                kw = dict(k=k, context=L - 1, reverse=reverse, **elig)
                _equal(eng.score_path_topk(rows, cols, L, unit, radius=0, **kw), eng.score_seq_topk(rows, cols, L, **kw),
                       ("radius 0", L, kw))
                _equal(eng.score_path_topk(rows, cols, L, unit, radius=10, **kw),
                       eng.score_peak_topk(rows, cols, 10, seq_len=L, **kw), ("radius 10", L, kw))
                need = eng.score_path_topk_workspace_bytes(300, 517, L, 1, k=k, context=L - 1, reverse=reverse,
                                                           causal=elig.get("causal", False))
                assert need == eng.score_seq_topk_workspace_bytes(300, 517, L, k=k, context=L - 1, reverse=reverse,
                                                                  causal=elig.get("causal", False))
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 3. one block
def _reference(e, rows, cols, L, paths, k, radius=0, window=-1, row0=0, causal=False, row_self=None, context=0,
               reverse="both", score=None):
    """score_all_pairs -> seq_path_filter -> (peak_filter ->) topk_rows_large on the same rectangle, codes gathered"""
    score = e.score_all_pairs(rows, cols) if score is None else score
    q, c = e.seq_path_filter(score, L, paths, context=context, reverse=reverse, want_code=True)
    rs = None if row_self is None else row_self[context:]
    elig = dict(row0=row0 + context, window=window, causal=causal, row_self=rs)
    x = e.peak_filter(q, radius, **elig) if radius > 0 else q
    v, i = e.topk_rows_large(x, k=k, **elig)
    codes = torch.where(i >= 0, c.gather(1, i.clamp(min=0).long()), torch.zeros_like(i, dtype=torch.uint8))
    return v, i, codes


@pytest.mark.parametrize("shape", [(37, 131), (300, 517)])
def test_pooled_equals_matrix_filter_selection(eng, shape):
    r, m = shape
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(r).permutation(m)[:r].astype(np.int32))
    modes = [dict(window=-1), dict(window=0), dict(window=50, causal=True), dict(window=10, row_self=perm),
             dict(window=10, causal=True, row_self=perm), dict(window=50, row0=120)]
    n = 0
    for L in (1, 2, 8, 32):
        sets = _path_sets(L)
        for ctx in sorted({0, L - 1}):
            for j, mode in enumerate(modes):
                k = (1, 4, 17, m + 5)[(j + n) % 4]
                reverse = DIRECTIONS[(j + n // 3) % 3]
                name, paths = sets[(j + n) % len(sets)]
                radius = (0, 10, 0, 3)[(j + n // 2) % 4]
                kw = dict(k=k, radius=radius, context=ctx, reverse=reverse, **mode)
                got = eng.score_path_topk(rows, cols, L, paths, **kw)
                _equal(got, _reference(eng, rows, cols, L, paths, score=score, **kw), (shape, L, name, kw))
                assert got[0].shape == (r - ctx, k)
            n += 1
    nine = seq_path_ref.seq_paths(8, seq_path_ref.SLOPES)
    codes = eng.score_path_topk(rows, cols, 8, nine, k=4, window=0)[2]
    assert len(torch.unique(codes)) >= 6                       # many paths, both directions, are listed somewhere
    # context == R: empty lists; no columns: padding only
    v, i, c = eng.score_path_topk(rows, cols, 8, nine, k=3, context=r)
    assert v.shape == (0, 3) and i.shape == (0, 3) and c.shape == (0, 3)
    v, i, c = eng.score_path_topk(rows, cols[:0], 8, nine, k=3, context=2, reverse=True, radius=5)
    assert v.shape == (r - 2, 3) and (v == -float("inf")).all() and (i == -1).all() and not c.any()
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 4. several blocks
def test_several_blocks_tuned_handle(eng):
    m, r, L = M_A, RB_A + 1, 8
    rb = _seq_rb(r, m, L)
    assert rb < r                                              # more than one block runs
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    a256 = lambda v: (v + 255) & ~255
    base = eng.score_seq_topk_workspace_bytes(r, m, L, k=17, reverse=True)
    assert eng.score_path_topk_workspace_bytes(r, m, L, 9, k=17, reverse=True) == base + a256(rb * m)
    assert eng.score_path_topk_workspace_bytes(r, m, L, 9, k=17) == eng.score_seq_topk_workspace_bytes(r, m, L, k=17)
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(r).integers(0, m, size=r).astype(np.int32))
    for kw in (dict(k=17, window=50, context=L - 1), dict(k=4, window=5, row0=7, causal=True, reverse=True, radius=10),
               dict(k=1, window=10, causal=True, row_self=perm, reverse=False, context=3)):
        got = eng.score_path_topk(rows, cols, L, nine, **kw)
        _equal(got, _reference(eng, rows, cols, L, nine, score=score, **kw), ("tuned, blocks", kw))
    eng.check_status()


def test_several_blocks_thin(eng):
    m, r, L = 262144, 70, 32
    assert _seq_rb(r, m, L) == 33 < r                          # the context nearly fills a block: 31 + 33 rows of 1 MB
    paths = _path_sets(L)[2][1]                                # the jump of 64: the widest halo, the deepest LDS tile
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    kw = dict(k=4, window=50, context=L - 1)
    _equal(eng.score_path_topk(rows, cols, L, paths, **kw), _reference(eng, rows, cols, L, paths, **kw), ("thin", kw))
    eng.check_status()


def test_several_blocks_wide_checkpoint(sd):
    from sg_pr_amd import engine
    m, r, L = M_A, RB_A + 1, 8
    assert _seq_rb(r, m, L) < r
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    wide = engine.Engine(_wide_checkpoint(sd), device=0)
    try:
        assert not wide.uses_f16_planes()
        rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
        kw = dict(k=17, window=50, context=L - 1)
        _equal(wide.score_path_topk(rows, cols, L, nine, **kw), _reference(wide, rows, cols, L, nine, **kw),
               ("wide checkpoint", kw))
        wide.check_status()
    finally:
        wide.close()


def test_several_blocks_any_shape():
    m, r, L = M_A, RB_A + 1, 8
    assert _seq_rb(r, m, L) < r
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    any_eng = _any_shape(_any_shape())
    try:
        assert any_eng.any_shape
        rows, cols = _pooled(r, 48, 1.0, r + 1), _pooled(m, 48, 1.0, m + 1)
        kw = dict(k=17, window=50, causal=True, context=2, radius=10)
        _equal(any_eng.score_path_topk(rows, cols, L, nine, **kw), _reference(any_eng, rows, cols, L, nine, **kw),
               ("any-shape", kw))
        any_eng.check_status()
    finally:
        any_eng.close()


# ------------------------------------------------------------------------------------------------- 5. statelessness
def test_dirty_workspaces(eng):
    rows, cols = _pooled(300, 32, 3.0, 5), _pooled(4541, 32, 3.0, 6)
    score = torch.from_numpy(_scores(300, 4541, 13)).cuda()
    nine = seq_path_ref.seq_paths(8, seq_path_ref.SLOPES)
    base = _check_all_patterns(eng, lambda: eng.score_path_topk(rows, cols, 8, nine, k=100, window=50, causal=True,
                                                                context=7), "score_path_topk")
    assert base[0].shape == (293, 100)
    _check_all_patterns(eng, lambda: eng.score_path_topk(rows, cols, 8, nine, k=3, radius=10, window=50, reverse=True),
                        "score_path_topk, one direction, radius 10")
    _check_all_patterns(eng, lambda: eng.seq_path_filter(score, 8, nine, reverse="both", want_code=True), "seq_path_filter")


def test_two_streams_write_prefilled_outputs(eng):
    lib, h = eng.lib, eng._h
    rows_a, cols_a = _pooled(300, 32, 3.0, 31), _pooled(1200, 32, 3.0, 32)
    rows_b, cols_b = _pooled(250, 32, 3.0, 33), _pooled(2100, 32, 3.0, 34)
    block = eng.score_all_pairs(rows_b, cols_b)
    ka, kb = 8, 3
    nine = np.ascontiguousarray(seq_path_ref.seq_paths(8, seq_path_ref.SLOPES))
    two = np.ascontiguousarray(seq_path_ref.seq_paths(4, ["1", "2"]))
    want_a = eng.score_path_topk(rows_a, cols_a, 8, nine, k=ka, radius=10, window=20, context=7, reverse="both")
    want_b = eng.score_path_topk(rows_b, cols_b, 4, two, k=kb, window=5, causal=True, row0=900, reverse=True)
    want_q = eng.seq_path_filter(block, 8, nine, context=7, reverse="both", want_code=True)
    na = eng.score_path_topk_workspace_bytes(300, 1200, 8, 9, k=ka, radius=10, context=7, reverse="both")
    nb = eng.score_path_topk_workspace_bytes(250, 2100, 4, 2, k=kb, causal=True, reverse=True)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        va, ia, ca = _ff(293 * ka, torch.float32), _ff(293 * ka, torch.int32), _ff(293 * ka, torch.uint8)
        vb, ib, cb = _ff(250 * kb, torch.float32), _ff(250 * kb, torch.int32), _ff(250 * kb, torch.uint8)
        qb, qc = _ff(243 * 2100, torch.float32), _ff(243 * 2100, torch.uint8)
        wsa, wsb = _ff(na, torch.uint8), _ff(nb, torch.uint8)
        torch.cuda.synchronize()
        rc_a = lib.sgpr_score_path_topk(h, _dptr(rows_a), 300, _dptr(cols_a), 1200, 7, None, 0, 20, 2 | 4, 8,
                                        nine.ctypes.data, 9, 10, ka, _dptr(va), _dptr(ia), _dptr(ca), _dptr(wsa), na,
                                        ctypes.c_void_p(sa.cuda_stream))
        scratch = two.copy()                                  # the table is free to reuse once the call has returned
        rc_b = lib.sgpr_score_path_topk(h, _dptr(rows_b), 250, _dptr(cols_b), 2100, 0, None, 900, 5, 1 | 4, 4,
                                        scratch.ctypes.data, 2, 0, kb, _dptr(vb), _dptr(ib), _dptr(cb), _dptr(wsb), nb,
                                        ctypes.c_void_p(sb.cuda_stream))
        scratch[:] = 0
        rc_q = lib.sgpr_seq_path_filter(h, _dptr(block), 250, 2100, 2100, 7, 8, 2 | 4, nine.ctypes.data, 9, _dptr(qb), 2100,
                                        _dptr(qc), ctypes.c_void_p(sb.cuda_stream))
        torch.cuda.synchronize()
        assert (rc_a, rc_b, rc_q) == (0, 0, 0), lib.sgpr_last_error()
        _equal((va.view(293, ka), ia.view(293, ka), ca.view(293, ka)), want_a, "stream a")
        _equal((vb.view(250, kb), ib.view(250, kb), cb.view(250, kb)), want_b, "stream b")
        _equal((qb.view(243, 2100), qc.view(243, 2100)), want_q, "stream b, filter")
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 6. the planted case
@pytest.mark.parametrize("slope", PLANTED_SLOPES, ids=["%d/%d" % s for s in PLANTED_SLOPES])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_revisits_on_the_device(eng, seed, slope):
    L = 8
    s, col = seq_path_ref.planted(seed, slope)
    dev = torch.from_numpy(s).cuda()
    paths = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    fwd, rev = np.arange(200 + L, 300), np.arange(300 + L, 400)

    def rates(q):
        best = eng.topk_rows_large(q, k=1, window=50)[1][:, 0].cpu().numpy()
        return float(np.mean(best[fwd] == col[fwd])), float(np.mean(best[rev] == col[rev]))

    uf, ur = rates(eng.seq_filter(dev, L, reverse="both"))
    q, code = eng.seq_path_filter(dev, L, paths, reverse="both", want_code=True)
    pf, pr = rates(q)
    code = code.cpu().numpy()
    right = float(np.concatenate([(code[fwd, col[fwd]] & 1) == 0, (code[rev, col[rev]] & 1) == 1]).mean())
    print("seed", seed, "slope", slope, "unit diagonal:", uf, ur, "path set:", pf, pr, "direction bit right:", right)
    assert uf <= 0.15 and ur <= 0.15
    assert pf >= 0.75 and pr >= 0.75
    assert right >= 0.95
    # ... and they are the host test's figures: the device filter is the reference
    hq, hc = seq_path_ref.path_filter(s, paths, 0, True, True)
    assert (uf, ur, pf, pr, right) == planted_figures(s, col, seq_ref.seq_filter(s, L, 0, True, True)[0], hq, hc, L)


# ------------------------------------------------------------------------------------------------- 7. online = offline
def test_place_database_online_equals_offline(model):
    """query_seq(slopes=) before every append (causal, L = 8, k = 4) against one score_path_topk call over the whole
    sequence, with window = the paths' largest offset: no reverse sum of an eligible column reaches a frame that is not
    in the database yet."""
    from sg_pr_amd import engine
    from sg_pr_amd.place_db import PlaceDatabase
    n, L, k = 120, 8, 4
    paths = engine.seq_paths(L, seq_path_ref.SLOPES)
    window = int(paths.max())
    assert window == 14
    pooled = _pooled(n, 32, 3.0, 77)
    db = PlaceDatabase(model, capacity=4)
    got = []
    for t in range(n):
        got.append(db.query_seq(None, None, L, k=k, window=window, causal=True, pooled=pooled[t:t + 1],
                                slopes=seq_path_ref.SLOPES))
        db.append_pooled(pooled[t:t + 1])
    online = tuple(torch.cat([g[j] for g in got]) for j in range(3))
    e = model.engine()
    offline = e.score_path_topk(pooled, pooled, L, paths, k=k, window=window, causal=True)
    _equal(online, offline, "online / offline")
    assert (offline[1][:window + 1] == -1).all() and (offline[1][window + k:] >= 0).all()
    assert len(torch.unique(offline[2])) >= 6
    # a run of members, with and without distinct
    run = db.query_ids_seq(40, 30, L, k=k, window=window, slopes=seq_path_ref.SLOPES)
    want = e.score_path_topk(pooled, pooled, L, paths, k=k, window=window)
    _equal(run, tuple(w[40:70] for w in want), "query_ids_seq")
    run = db.query_ids_seq(40, 30, L, k=k, window=window, slopes=seq_path_ref.SLOPES, distinct=5)
    want = e.score_path_topk(pooled, pooled, L, paths, k=k, window=window, radius=5)
    _equal(run, tuple(w[40:70] for w in want), "query_ids_seq, distinct")
    e.check_status()


# ------------------------------------------------------------------------------------------------- 8. the Python surface
def test_loop_closures_seq_slopes(model):
    from sg_pr_amd import engine
    e = model.engine()
    pooled = _pooled(150, 32, 3.0, 78)
    for kw in (dict(k=4, window=16), dict(k=4, window=16, seq_len=8), dict(k=2, window=16, causal=True, seq_len=8, seq_reverse=False),
               dict(k=3, window=16, seq_len=8, distinct=5), dict(k=3, window=16, distinct=5)):
        base = model.loop_closures(pooled, pooled, **kw)
        same = model.loop_closures(pooled, pooled, seq_slopes=None, **kw)    # the default: today's path and results
        _equal(same, base, ("seq_slopes=None", kw))
    L = 8
    elig = dict(k=4, window=16)
    _equal(model.loop_closures(pooled, pooled, seq_len=L, **elig), e.score_seq_topk(pooled, pooled, L, **elig), "today, seq")
    _equal(model.loop_closures(pooled, pooled, seq_len=L, distinct=5, **elig),
           e.score_peak_topk(pooled, pooled, 5, seq_len=L, reverse="both", **elig), "today, distinct")
    paths = engine.seq_paths(L, ["1", "1/2", "2"])
    _equal(model.loop_closures(pooled, pooled, seq_len=L, seq_slopes=["1", (1, 2), "2"], **elig),
           e.score_path_topk(pooled, pooled, L, paths, **elig), "seq_slopes")
    _equal(model.loop_closures(pooled, pooled, seq_len=L, seq_slopes=["1", (1, 2), "2"], distinct=5, seq_reverse=True, **elig),
           e.score_path_topk(pooled, pooled, L, paths, radius=5, reverse=True, **elig), "seq_slopes, distinct")
    # the unit slope alone: today's lists, the code being the direction
    _equal(model.loop_closures(pooled, pooled, seq_len=L, seq_slopes=["1"], **elig),
           e.score_seq_topk(pooled, pooled, L, **elig), "seq_slopes = 1")
    with pytest.raises(ValueError):
        model.loop_closures(pooled, pooled, seq_slopes=["1", "2"], **elig)   # seq_len = 1
    with pytest.raises(ValueError):
        model.loop_closures(pooled, pooled, seq_len=L, seq_slopes=["10"], **elig)


# ------------------------------------------------------------------------------------------------- 9. the tools
def test_place_db_cli_seq_slopes(model, tmp_path, ckpt_path, capsys):
    from sg_pr_amd import engine, graph_store, place_db, synth
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
    paths = engine.seq_paths(8, seq_path_ref.SLOPES)
    for extra, radius in (([], 0), (["--distinct", "5"], 5)):
        place_db.main([str(cfg), "--k", "3", "--window", "14", "--seq-len", "8", "--seq-slopes", "1,1/2,2/3,3/2,2"] + extra)
        line = next(l for l in capsys.readouterr().out.splitlines() if "share of listed entries per path" in l)
        assert "recall@1" in line and "recall@3" in line and "unit slope" in line and "paths 9" in line, line
        z = np.load(tmp_path / "eva" / "07_slopes.npz")
        assert sorted(z.files) == sorted(["frame", "indices", "scores", "codes", "paths", "recall", "seq_len"] +
                                         (["radius"] if radius else []))
        v, i, c = eng.score_path_topk(pooled, pooled, 8, paths, k=3, radius=radius, window=14)
        assert np.array_equal(z["indices"], i.cpu().numpy()) and np.array_equal(z["codes"], c.cpu().numpy())
        assert np.array_equal(z["scores"].view(np.uint32), v.cpu().numpy().view(np.uint32))
        assert np.array_equal(z["paths"], paths) and int(z["seq_len"]) == 8 and z["recall"].shape == (3,)
        listed = z["indices"] >= 0
        share = np.bincount(z["codes"][listed] >> 1, minlength=9) / listed.sum()
        assert " ".join("%.3f" % x for x in share) in line
        unit = np.load(tmp_path / "eva" / ("07_distinct.npz" if radius else "07_topk.npz"))     # still written
        assert "recall@1 %.4f (unit slope %.4f)" % (z["recall"][0], unit["recall"][0]) in line
    place_db.main([str(cfg), "--k", "3", "--window", "14", "--seq-len", "8"])       # without the flag: as before
    assert sorted(np.load(tmp_path / "eva" / "07_topk.npz").files) == ["dirs", "frame", "indices", "recall", "scores", "seq_len"]
    for bad in (["--seq-slopes", "1,2"], ["--seq-len", "8", "--seq-slopes", "1,x"], ["--seq-len", "8", "--seq-slopes", "10"]):
        with pytest.raises(SystemExit):
            place_db.main([str(cfg)] + bad)


def test_path_bench_tool(capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import path_bench
    recs = path_bench.main(["--tiny"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert lines == recs
    recall = [r for r in recs if "recall1_paths" in r]
    assert {(r["case"], r["seq_len"]) for r in recall} == {(c, L) for c in ("slope 2", "slope 1/2") for L in (8, 16)}
    assert all(0.0 <= r[f] <= 1.0 for r in recall for f in ("recall1_single", "recall1_unit", "recall1_paths"))
    assert all(r["paths"] == 9 and abs(sum(r["share_per_path"]) - 1.0) < 0.01 for r in recall)
    calls = [r for r in recs if "path_ms" in r]
    assert {(r["seq_len"], r["k"]) for r in calls} == {(L, k) for L in (8, 16) for k in (1, 16)}
    assert all(r["path_ms"] > 0 and r["seq_ms"] > 0 and r["path_over_seq"] > 0 and r["path_peak_mb"] > 0
               and r["seq_peak_mb"] > 0 for r in calls)
    filt = [r for r in recs if "filter_ms" in r]
    assert len(filt) == 6 and all(r["filter_ms"] > 0 and r["copy_ms"] > 0 for r in filt)
