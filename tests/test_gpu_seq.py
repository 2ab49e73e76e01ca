"""sgpr_seq_filter / sgpr_score_seq_topk on the GPU: the diagonal filter against the NumPy reference bit for bit, the
pooled form against score_all_pairs -> seq_filter -> topk_rows_large on the same rectangle (one block and several, on
every kind of handle), dirty workspaces, the planted revisit, the place database online against one offline call, and
the two command-line tools."""
import os

import numpy as np
import pytest
import torch

import score_ref
import seq_ref
from test_gpu_row_blocks import M_A, RB_A, _rb, _rows_quantity, _scale_row
from test_gpu_score_range import _any_shape, _wide_checkpoint
from test_gpu_stateless import _check_all_patterns

pytestmark = pytest.mark.gpu

SEQ_TR, SEQ_TC = 32, 256          # seq_filter_kernel's tile (sgpr_seq.hip): output rows x columns
LENGTHS = (1, 2, 3, 8, 31, 32)
DIRECTIONS = (False, True, "both")


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


def _pooled(n, width, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, width, generator=g) * scale).cuda()


def _scores(r, m, seed, ld=None):
    """test_gpu_topk_large._scores without its subnormals: SG-PR-like rows, 60 % of the entries quantised to 1/64 (their
    sums are exact, so equal forward and reverse means occur), a constant patch, -0.0 next to +0.0, +-inf and NaN;
    ld > m gives a strided view -> host float32 array [r, ld]"""
    rng = np.random.default_rng(seed)
    ld = ld or m
    s = (1.0 - np.exp(rng.standard_normal((r, ld)) * 2.0 - 6.0)).astype(np.float32)
    s = np.where(rng.random((r, ld)) < 0.15, rng.random((r, ld), dtype=np.float32), s)
    s = np.where(rng.random((r, ld)) < 0.6, np.round(s * 64.0) / 64.0, s).astype(np.float32)
    s[r // 3:r // 3 + 6, m // 4:m // 4 + 40] = 0.5
    flat = s.reshape(-1)
    n = r * ld
    for val, frac in ((0.0, 0.002), (-0.0, 0.004), (np.inf, 0.0005), (-np.inf, 0.001), (np.nan, 0.002), (-5.0, 0.001)):
        flat[rng.integers(0, n, size=max(1, int(n * frac)))] = val
    return s


def _same_bits(got, want, what):
    """float arrays: NaN where the reference has NaN, the same bit pattern everywhere else"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _equal(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, j, g.shape, w.shape, g.dtype, w.dtype)
        gv = g.view(torch.int32) if g.dtype == torch.float32 else g
        wv = w.view(torch.int32) if w.dtype == torch.float32 else w
        bad = gv != wv
        assert not bad.any(), (what, "output", j, bad.nonzero()[:5].tolist(), int(bad.sum()))


def _flags(reverse):
    return dict(forward=reverse is not True, reverse=reverse is not False)


# ------------------------------------------------------------------------------------------------- 1. the filter
FILTER_SHAPES = [(1, 1, 0, 0), (5, 7, 0, 0), (37, 131, 0, 0), (70, 300, 3, 5),
                 (SEQ_TR + 1, SEQ_TC - 1, 0, 0), (SEQ_TR + 1, SEQ_TC + 1, 0, 0), (SEQ_TR + 1, 2 * SEQ_TC + 3, 0, 0)]


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=["%dx%d" % s[:2] for s in FILTER_SHAPES])
def test_filter_equals_the_reference(eng, shape):
    r, m, pad_in, pad_out = shape
    host = _scores(r, m, 7 * r + m, ld=m + pad_in)
    dev = torch.from_numpy(host).cuda()[:, :m]               # ld = m + pad_in: read in place
    assert dev.stride(0) == m + pad_in or r == 1
    ties = 0
    for L in LENGTHS:
        for reverse in DIRECTIONS:
            wq, wd = seq_ref.seq_filter(host[:, :m], L, 0, **_flags(reverse))
            if reverse == "both" and L > 1:
                f = seq_ref.seq_filter(host[:, :m], L, 0, True, False)[0]
                b = seq_ref.seq_filter(host[:, :m], L, 0, False, True)[0]
                ties += int(((f == b) & (np.arange(m)[None, :] > 0) & (np.arange(r)[:, None] > 0)).sum())
            for ctx in sorted({0, min(1, r), min(L - 1, r), r - 1}):
                ro = r - ctx
                out = torch.full((ro, m + pad_out), 7.0, device="cuda")
                odir = torch.full((ro, m + pad_out), 9, dtype=torch.uint8, device="cuda")
                q, d = eng.seq_filter(dev, L, context=ctx, reverse=reverse, out=out[:, :m], out_dir=odir[:, :m])
                what = (shape, L, reverse, ctx)
                _same_bits(q.cpu().numpy(), wq[ctx:], what)
                assert np.array_equal(d.cpu().numpy(), wd[ctx:]), what
                if pad_out:                                   # nothing written past column m of an output row
                    assert (out[:, m:] == 7.0).all() and (odir[:, m:] == 9).all(), what
                q2 = eng.seq_filter(dev, L, context=ctx, reverse=reverse)          # without dir
                _same_bits(q2.cpu().numpy(), wq[ctx:], what)
    if r > 30:
        assert ties > 0                                       # equal forward and reverse means away from the edges occur
    # context == R: an empty result
    assert eng.seq_filter(dev, 3, context=r).shape == (0, m)


# ------------------------------------------------------------------------------------------------- 2. L = 1
def test_length_one_forward_equals_score_topk_large(eng):
    rows, cols = _pooled(300, 32, 3.0, 1), _pooled(517, 32, 3.0, 2)
    for k in (1, 17):
        for window, causal in ((-1, False), (50, True)):
            want = eng.score_topk_large(rows, cols, k=k, window=window, row0=3, causal=causal)
            v, i, d = eng.score_seq_topk(rows, cols, 1, k=k, window=window, row0=3, causal=causal, reverse=False)
            _equal((v, i), want, ("L = 1", k, window, causal))
            assert not d.any()


# ------------------------------------------------------------------------------------------------- 3. one block
def _reference(e, rows, cols, L, k, window=-1, row0=0, causal=False, row_self=None, context=0, reverse="both", score=None):
    """score_all_pairs -> seq_filter -> topk_rows_large on the same rectangle, dirs gathered from the filter's dir"""
    score = e.score_all_pairs(rows, cols) if score is None else score
    q, d = e.seq_filter(score, L, context=context, reverse=reverse, want_dir=True)
    rs = None if row_self is None else row_self[context:]
    v, i = e.topk_rows_large(q, k=k, row0=row0 + context, window=window, causal=causal, row_self=rs)
    dirs = torch.where(i >= 0, d.gather(1, i.clamp(min=0).long()), torch.zeros_like(i, dtype=torch.uint8))
    return v, i, dirs


@pytest.mark.parametrize("shape", [(37, 131), (300, 517)])
def test_pooled_equals_matrix_filter_selection(eng, shape):
    r, m = shape
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(r).permutation(m)[:r].astype(np.int32))
    modes = [dict(window=-1), dict(window=0), dict(window=50), dict(window=50, causal=True), dict(window=-1, causal=True),
             dict(window=10, row_self=perm), dict(window=10, causal=True, row_self=perm), dict(window=50, row0=120),
             dict(window=0, row0=120, causal=True)]
    n = 0
    for L in (2, 8, 32):
        for ctx in (0, L - 1):
            for j, mode in enumerate(modes):
                k = (1, 4, 17, m + 5)[(j + n) % 4]
                reverse = DIRECTIONS[(j + n // 3) % 3]
                kw = dict(k=k, context=ctx, reverse=reverse, **mode)
                got = eng.score_seq_topk(rows, cols, L, **kw)
                _equal(got, _reference(eng, rows, cols, L, score=score, **kw), (shape, L, kw))
                assert got[0].shape == (r - ctx, k)
            n += 1
    # every k at every window, both directions, one length
    for k in (1, 4, 17, m + 5):
        for window in (-1, 0, 50):
            kw = dict(k=k, window=window, context=7)
            _equal(eng.score_seq_topk(rows, cols, 8, **kw), _reference(eng, rows, cols, 8, score=score, **kw), (shape, kw))
    both = eng.score_seq_topk(rows, cols, 8, k=4, window=0)[2]
    assert both.any() and not both.all()                       # both directions are taken somewhere
    # context == R: empty lists; no columns: padding only
    v, i, d = eng.score_seq_topk(rows, cols, 8, k=3, context=r)
    assert v.shape == (0, 3) and i.shape == (0, 3) and d.shape == (0, 3)
    v, i, d = eng.score_seq_topk(rows, cols[:0], 8, k=3, context=2, reverse=True)
    assert v.shape == (r - 2, 3) and (v == -float("inf")).all() and (i == -1).all() and not d.any()
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 4. several blocks
def _seq_rb(r, m, L):
    """output rows per block: a block holds at most 64 MB including its L - 1 context rows"""
    return max(1, min(r, (64 << 20) // (4 * m) - (L - 1)))


BLOCK_CASES = [(M_A, RB_A + 1, 8), (262144, 150, 32)]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=["rb+1", "thin"])
def test_several_blocks_tuned_handle(eng, case):
    m, r, L = case
    rb = _seq_rb(r, m, L)
    assert rb < r                                              # more than one block runs
    if m == 262144:
        assert rb == 33 and L - 1 == 31                        # the context nearly fills a block: 31 + 33 rows of 1 MB
    assert eng.score_seq_topk_workspace_bytes(r, m, L, k=17) < 3.2 * (64 << 20) + 64 * m
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(r).integers(0, m, size=r).astype(np.int32))
    for kw in (dict(k=17, window=50, context=L - 1), dict(k=4, window=5, row0=7, causal=True, reverse=True),
               dict(k=1, window=10, causal=True, row_self=perm, reverse=False, context=3)):
        got = eng.score_seq_topk(rows, cols, L, **kw)
        _equal(got, _reference(eng, rows, cols, L, score=score, **kw), (case, kw))
    eng.check_status()


def test_several_blocks_wide_checkpoint(sd):
    from sg_pr_amd import engine
    m, r, L = M_A, RB_A + 1, 8
    assert _seq_rb(r, m, L) < r
    wide = engine.Engine(_wide_checkpoint(sd), device=0)
    try:
        assert not wide.uses_f16_planes()
        rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
        kw = dict(k=17, window=50, context=L - 1)
        _equal(wide.score_seq_topk(rows, cols, L, **kw), _reference(wide, rows, cols, L, **kw), ("wide checkpoint", kw))
        wide.check_status()
    finally:
        wide.close()


def test_several_blocks_any_shape():
    m, r, L = M_A, RB_A + 1, 8
    assert _seq_rb(r, m, L) < r
    any_eng = _any_shape(_any_shape())
    try:
        assert any_eng.any_shape
        rows, cols = _pooled(r, 48, 1.0, r + 1), _pooled(m, 48, 1.0, m + 1)
        kw = dict(k=17, window=50, causal=True, context=2)
        _equal(any_eng.score_seq_topk(rows, cols, L, **kw), _reference(any_eng, rows, cols, L, **kw), ("any-shape", kw))
        any_eng.check_status()
    finally:
        any_eng.close()


def test_f16_range_is_the_calls(eng, sd):
    """One row far outside the f16 range in the last block only: every block takes the datapath score_all_pairs takes on
    the whole rectangle."""
    m, L = 300, 8
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
    for kw in (dict(k=17, window=-1, context=L - 1), dict(k=4, window=5, row0=5, causal=True, reverse=True)):
        got = eng.score_seq_topk(rows, cols, L, **kw)
        _equal(got, _reference(eng, rows, cols, L, score=score, **kw), ("mixed range", kw))


# ------------------------------------------------------------------------------------------------- 5. statelessness
def test_dirty_workspaces(eng):
    rows, cols = _pooled(300, 32, 3.0, 5), _pooled(4541, 32, 3.0, 6)
    score = torch.from_numpy(_scores(300, 4541, 13)).cuda()
    base = _check_all_patterns(eng, lambda: eng.score_seq_topk(rows, cols, 8, k=100, window=50, causal=True, context=7),
                               "score_seq_topk")
    assert base[0].shape == (293, 100)
    _check_all_patterns(eng, lambda: eng.score_seq_topk(rows, cols, 32, k=1, window=50, reverse=True), "score_seq_topk, k 1")
    _check_all_patterns(eng, lambda: eng.seq_filter(score, 8, reverse="both", want_dir=True), "seq_filter")


# ------------------------------------------------------------------------------------------------- 6. the planted case
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_revisits_on_the_device(eng, seed):
    s, col = seq_ref.planted(seed)
    dev = torch.from_numpy(s).cuda()
    fwd, rev = np.arange(208, 300), np.arange(308, 400)

    def rates(q):
        best = eng.topk_rows_large(q, k=1, window=50)[1][:, 0].cpu().numpy()
        return float(np.mean(best[fwd] == col[fwd])), float(np.mean(best[rev] == col[rev]))

    one_f, one_r = rates(dev)
    ff, fr = rates(eng.seq_filter(dev, 8, reverse=False))
    rf, rr = rates(eng.seq_filter(dev, 8, reverse=True))
    qb, db = eng.seq_filter(dev, 8, reverse="both", want_dir=True)
    bf, br = rates(qb)
    print("seed", seed, "L = 1:", one_f, one_r, "forward:", ff, fr, "reverse:", rf, rr, "both:", bf, br)
    assert one_f <= 0.55 and one_r <= 0.55
    assert ff >= 0.90 and rr >= 0.90
    assert fr <= 0.05 and rf <= 0.05
    assert bf >= 0.85 and br >= 0.85
    db = db.cpu().numpy()
    assert not db[fwd, col[fwd]].any() and db[rev, col[rev]].all()
    # ... and they are the host test's figures: the device filter is the reference
    assert (ff, fr) == seq_ref.planted_rates(seq_ref.seq_filter(s, 8, 0, True, False)[0], col)
    assert (bf, br) == seq_ref.planted_rates(seq_ref.seq_filter(s, 8, 0, True, True)[0], col)


# ------------------------------------------------------------------------------------------------- 7. online = offline
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
    """query_seq before every append (causal, L = 8, k = 4; window 10 >= L - 1, so no reverse sum of an eligible column
    reaches a frame that is not in the database yet) against one score_seq_topk call over the whole sequence."""
    from sg_pr_amd.place_db import PlaceDatabase
    n, L, k, window = 120, 8, 4, 10
    pooled = _pooled(n, 32, 3.0, 77)
    db = PlaceDatabase(model, capacity=4)
    got = []
    for t in range(n):
        got.append(db.query_seq(None, None, L, k=k, window=window, causal=True, pooled=pooled[t:t + 1]))
        db.append_pooled(pooled[t:t + 1])
    online = tuple(torch.cat([g[j] for g in got]) for j in range(3))
    offline = model.engine().score_seq_topk(pooled, pooled, L, k=k, window=window, causal=True)
    _equal(online, offline, "online / offline")
    assert (offline[1][:window + 1] == -1).all() and (offline[1][window + k:] >= 0).all()
    assert offline[2].any() and not offline[2].all()
    # a run of members, and model.loop_closures' route to the same call
    run = db.query_ids_seq(40, 30, L, k=k, window=window)
    want = model.engine().score_seq_topk(pooled, pooled, L, k=k, window=window)
    _equal(run, tuple(w[40:70] for w in want), "query_ids_seq")
    _equal(model.loop_closures(pooled, pooled, k=k, window=window, seq_len=L), want, "loop_closures seq_len")
    _equal(model.loop_closures(pooled, pooled, k=k, window=window), model.engine().score_topk(pooled, pooled, k=k, window=window),
           "loop_closures seq_len = 1")
    model.engine().check_status()


# ------------------------------------------------------------------------------------------------- 8. the tools
def test_command_line_tools(model, tmp_path, ckpt_path):
    from sg_pr_amd import allpairs, graph_store, metrics, place_db, synth
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
    place_db.main([str(cfg), "--k", "3", "--window", "10", "--seq-len", "8"])
    z = np.load(tmp_path / "eva" / "07_topk.npz")
    assert sorted(z.files) == ["dirs", "frame", "indices", "recall", "scores", "seq_len"]
    assert int(z["seq_len"]) == 8 and z["dirs"].shape == z["indices"].shape == z["scores"].shape == (n, 3)
    assert z["dirs"].dtype == np.uint8 and z["recall"].shape == (3,)
    eng = model.engine()
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    v, i, d = eng.score_seq_topk(pooled, pooled, 8, k=3, window=10)
    assert np.array_equal(z["indices"], i.cpu().numpy()) and np.array_equal(z["dirs"], d.cpu().numpy())
    assert np.array_equal(z["scores"].view(np.uint32), v.cpu().numpy().view(np.uint32))
    place_db.main([str(cfg), "--k", "3", "--window", "10", "--seq-len", "8", "--seq-reverse", "on"])
    z = np.load(tmp_path / "eva" / "07_topk.npz")
    assert z["dirs"][z["indices"] >= 0].all()
    place_db.main([str(cfg), "--k", "3", "--window", "10"])                         # without the flag: as before
    assert sorted(np.load(tmp_path / "eva" / "07_topk.npz").files) == ["frame", "indices", "recall", "scores"]

    res = graph_store.main([str(cfg), "--seq-len", "8"])
    r = graph_store.evaluate_all_pairs(model, seq, p_thresh=3.0, seq_len=8)
    assert res["07"] == r["f1_max"]
    with open(tmp_path / "eva" / "07_seq_F1_max.txt") as f:
        reported = float(f.read())
    assert reported == r["seq_f1_max"]
    host_q = seq_ref.seq_filter(r["matrix"].cpu().numpy(), 8, 0, True, True)[0]
    _same_bits(r["seq_matrix"].cpu().numpy(), host_q, "seq_matrix")
    gt, valid = allpairs.ground_truth_mask(allpairs.pose_distance_matrix(poses), 3)
    want = metrics.f1_max(gt[valid].numpy(), torch.from_numpy(host_q)[valid].numpy())
    assert abs(reported - want) < 1e-12
    lc = np.load(tmp_path / "eva" / "07_seq_loop_closures.npy")
    assert lc.shape == (n, 3)
    with pytest.raises(ValueError, match="keep_matrix"):
        graph_store.evaluate_all_pairs(model, seq, p_thresh=3.0, seq_len=8, keep_matrix=False)
