"""sgpr_score_above / sgpr_rows_above: every pair scoring at or above a threshold, straight from pooled vectors (fused
two-pass tail, no matrix), on every handle kind, and the layers above it (op, place database, CLI, two ranks) - every
result against the same handle's score_all_pairs matrix, masked and filtered with torch, bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def eng(ckpt_path):
    from sg_pr_amd import engine
    from oracle import sgpr_oracle
    e = engine.Engine(sgpr_oracle.load_checkpoint(ckpt_path), device=0)
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


@pytest.fixture(scope="module")
def kitti_pooled(eng):
    from sg_pr_amd import synth
    centers, labels, _, _ = synth.kitti_like_sequence(4541, 100, seed=3)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    return pooled


def _pooled(n, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 32, generator=g) * scale).cuda()


def _reference(score, thr, window=-1, row0=0, causal=False, row_self=None):
    """The dense matrix with the ineligible cells (and NaN) masked, >= thr, torch.nonzero (row-major)."""
    r, m = score.shape
    self_ = (torch.arange(r, device=score.device) + row0) if row_self is None else row_self.to(score.device).long()
    c = torch.arange(m, device=score.device)
    ok = (score >= thr) & ~torch.isnan(score)
    if window >= 0:
        ok &= (c[None, :] - self_[:, None]).abs() > window
    if causal:
        ok &= c[None, :] < self_[:, None]
    nz = torch.nonzero(ok)
    rp = torch.zeros(r + 1, dtype=torch.int64, device=score.device)
    rp[1:] = torch.cumsum(ok.sum(dim=1), 0)
    return nz[:, 0].to(torch.int32), nz[:, 1].to(torch.int32), score[ok], rp


def _equal(got, want, what):
    assert len(got) == 4
    for name, g, w in zip(("rows", "cols", "values", "row_ptr"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert torch.equal(g, w), (what, name)


def _quantile(score, q):
    v = score[~torch.isnan(score)].flatten().sort().values
    return float(v[min(v.numel() - 1, int(q * (v.numel() - 1)))])


def _check(e, rows, cols, thr, window=-1, row0=0, causal=False, row_self=None, score=None, what=()):
    score = e.score_all_pairs(rows, cols) if score is None else score
    want = _reference(score, thr, window, row0, causal, row_self)
    got = e.score_above(rows, cols, thr, window=window, row0=row0, causal=causal, row_self=row_self)
    _equal(got, want, ("score_above", thr, window, row0, causal) + tuple(what))
    got = e.rows_above(score, thr, window=window, row0=row0, causal=causal, row_self=row_self)
    _equal(got, want, ("rows_above", thr, window, row0, causal) + tuple(what))
    return want


@pytest.mark.parametrize("shape", [(37, 131), (1, 4541), (300, 517)])
def test_above_equals_masked_matrix(eng, shape):
    r, m = shape
    rows, cols = _pooled(r, r), _pooled(m, m + 1)
    score = eng.score_all_pairs(rows, cols)
    thrs = [_quantile(score, 0.5), _quantile(score, 0.99), -INF, INF]
    thrs.append(float(score[r // 2, m // 3]))             # an existing value: the comparison is inclusive
    for thr in thrs:
        for window in (-1, 0, 10, 50):
            for row0 in (0, 120):
                for causal in (False, True):
                    _check(eng, rows, cols, thr, window, row0, causal, score=score, what=shape)
    # the inclusive edge, explicitly: the pair holding the threshold value is reported, one ulp above it is not
    v = float(score[r // 2, m // 3])
    got = eng.score_above(rows, cols, v)
    assert bool(((got[0] == r // 2) & (got[1] == m // 3)).any())
    nxt = float(np.nextafter(np.float32(v), np.float32(2)))
    got = eng.score_above(rows, cols, nxt)
    assert not bool(((got[0] == r // 2) & (got[1] == m // 3)).any())


def test_full_kitti_like_set(eng, kitti_pooled):
    score = eng.score_all_pairs(kitti_pooled, kitti_pooled)
    for q in (1 - 1e-3, 1 - 1e-5):
        thr = _quantile(score, q)
        for window in (-1, 50):
            for causal in (False, True):
                want = _check(eng, kitti_pooled, kitti_pooled, thr, window, 0, causal, score=score, what=(q,))
                assert want[0].numel() > 0
    _check(eng, kitti_pooled, kitti_pooled, -INF, 50, 0, True, score=score)        # ~10 M pairs
    # repeated calls: identical bytes
    a = eng.score_above(kitti_pooled, kitti_pooled, _quantile(score, 0.999), window=50)
    for _ in range(3):
        b = eng.score_above(kitti_pooled, kitti_pooled, _quantile(score, 0.999), window=50)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_duplicates_nan_and_empty(eng):
    rows, cols = _pooled(40, 5), _pooled(300, 6)
    cols[100:141] = cols[7]                          # 41 duplicated columns: 42 equal scores per row
    cols[250] = float("nan")
    rows[3] = float("nan")
    score = eng.score_all_pairs(rows, cols)
    # the NaN graphs really are NaN in the matrix (not scored like a healthy graph upstream)
    assert torch.isnan(score[3]).all() and torch.isnan(score[:, 250]).all()
    for r in (0, 17):
        thr = float(score[r, 7])
        for window in (-1, 10):
            want = _check(eng, rows, cols, thr, window, score=score)
            assert int((want[0] == r).sum()) >= 1
    assert not torch.isnan(eng.score_above(rows, cols, -INF)[2]).any()
    want = _check(eng, rows, cols, -INF, score=score)
    assert want[0].numel() == int((~torch.isnan(score)).sum())     # every pair with a non-NaN score
    assert want[0].numel() == 39 * 299                             # = every pair of two healthy graphs, counted from the plant
    assert (want[0] != 3).all() and (want[1] != 250).all()
    # empty shapes: R = 0, M = 0
    for r, m in ((0, 50), (5, 0), (0, 0)):
        got = eng.score_above(rows[:r].contiguous(), cols[:m].contiguous(), 0.5, window=3)
        assert got[0].numel() == 0 and got[3].shape == (r + 1,) and int(got[3].abs().sum()) == 0
        got = eng.rows_above(torch.empty(r, m, device="cuda"), 0.5)
        assert got[0].numel() == 0 and got[3].shape == (r + 1,) and int(got[3].abs().sum()) == 0


def test_overflow_and_count_only(eng, kitti_pooled):
    rows, cols = kitti_pooled[:600].contiguous(), kitti_pooled
    score = eng.score_all_pairs(rows, cols)
    thr = _quantile(score, 0.99)
    want = _reference(score, thr, 50, 0, True)
    n = want[0].numel()
    assert n > 100
    for cap in (0, 1, 37, n // 2, n - 1, n, n + 5):
        for fn in ("score_above", "rows_above"):
            arg = (rows, cols) if fn == "score_above" else (score,)
            got = getattr(eng, fn)(*arg, thr, window=50, causal=True, capacity=cap)
            assert got[0].shape == (cap,)
            assert torch.equal(got[3], want[3]), (fn, cap)              # exact counts whatever the capacity
            k = min(cap, n)
            for g, w in zip(got[:3], want[:3]):
                assert torch.equal(g[:k], w[:k]), (fn, cap)
    eng.check_status()


def test_without_a_row_pointer(eng, kitti_pooled):
    """d_row_ptr NULL: the row pointer lives in the workspace; the pairs and the count are the same."""
    from sg_pr_amd.engine import _ptr
    rows, cols = kitti_pooled[:500].contiguous(), kitti_pooled
    want = eng.score_above(rows, cols, 0.95, window=50)
    n = want[0].numel()
    out = [torch.empty(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32)]
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws_bytes = eng.score_above_workspace_bytes(500, cols.shape[0])
    ws = eng._ws(ws_bytes)
    rc = eng.lib.sgpr_score_above(eng._h, _ptr(rows), 500, _ptr(cols), cols.shape[0], None, 0, 50, 0, 0.95,
                                  _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), n, None, _ptr(count), _ptr(ws), ws_bytes,
                                  eng._stream())
    eng._check(rc)
    assert int(count) == n
    for g, w in zip(out, want[:3]):
        assert torch.equal(g, w)


def test_row_blocks_of_a_long_launch(eng, kitti_pooled):
    """More rows than one fused launch takes (131072): the second block's positions continue from the first's count."""
    n = 131072 + 37
    pick = torch.arange(n, device="cuda") % kitti_pooled.shape[0]
    rows = kitti_pooled[pick].contiguous()
    cols = kitti_pooled[:300].contiguous()
    score = eng.score_all_pairs(rows, cols)
    thr = _quantile(score[:4541], 0.99)
    for causal in (False, True):
        want = _reference(score, thr, 5, 0, causal)
        _equal(eng.score_above(rows, cols, thr, window=5, causal=causal), want, ("blocks", causal))
        k = int(want[3][131072]) + 3                 # a capacity that ends inside the second block
        got = eng.score_above(rows, cols, thr, window=5, causal=causal, capacity=k)
        assert torch.equal(got[3], want[3])
        for g, w in zip(got[:3], want[:3]):
            assert torch.equal(g, w[:k])
    assert eng.score_above_workspace_bytes(300000, 300000) < 0.5e9


def test_row_self_and_its_out_of_range_report(eng, kitti_pooled):
    from sg_pr_amd.engine import SgprError
    rows, cols = kitti_pooled[:700].contiguous(), kitti_pooled[:2000].contiguous()
    score = eng.score_all_pairs(rows, cols)
    thr = _quantile(score, 0.99)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(2000)[:700].astype(np.int32))
    for causal in (False, True):
        for window in (-1, 20):
            _check(eng, rows, cols, thr, window, causal=causal, row_self=perm, score=score)
    eng.check_status()
    bad = torch.tensor([0, 3, 2000, 1], dtype=torch.int32)
    eng.score_above(rows[:4].contiguous(), cols, thr, row_self=bad)
    with pytest.raises(SgprError, match="row_self"):
        eng.check_status()
    eng.check_status()                                                    # the report was consumed


def test_range_guard_and_both_modes(eng, kitti_pooled):
    """x 1000: the exact fp32 per-pair path; x 0.25 / x 2: both forms of the f16 path - same bits as the matrix."""
    for scale, r, m in ((1000.0, 19, 300), (0.25, 300, 1200), (2.0, 300, 1200)):
        rows = (kitti_pooled[:r] * scale).contiguous()
        cols = (kitti_pooled[1000:1000 + m] * scale).contiguous()
        score = eng.score_all_pairs(rows, cols)
        for q in (0.5, 0.99):
            for causal in (False, True):
                _check(eng, rows, cols, _quantile(score, q), 5, 3, causal, score=score, what=(scale,))


def test_fallback_handles(eng, kitti_pooled, oracle_sd):
    """Debug bit 13 (three-plane tail), a wide-range checkpoint and an any-shape handle: bit-equal to their own matrix."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import score_ref
    from sg_pr_amd import engine, sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    rows, cols = kitti_pooled[:200].contiguous(), kitti_pooled[:900].contiguous()
    eng.set_skip_mask(1 << 13)
    try:
        score = eng.score_all_pairs(rows, cols)
        for causal in (False, True):
            _check(eng, rows, cols, _quantile(score, 0.98), 10, 0, causal, score=score, what=("bit 13",))
    finally:
        eng.set_skip_mask(0)
    rn, cn = rows.cpu().numpy(), cols.cpu().numpy()
    wide_sd = score_ref.dead_neuron_with_huge_fold(oracle_sd, [(rn, cn)])[0]
    ew = engine.Engine(wide_sd, device=0)
    try:
        score = ew.score_all_pairs(rows, cols)
        for causal in (False, True):
            _check(ew, rows, cols, _quantile(score, 0.98), 10, 0, causal, score=score, what=("wide",))
    finally:
        ew.close()
    args = sgpr_args()
    args.filters_1, args.filters_2, args.filters_3, args.tensor_neurons, args.bottle_neck_neurons = 64, 64, 48, 16, 16
    args.node_num, args.K = 64, 10
    torch.manual_seed(5)
    m = sg_net.SG(args, 12).eval()
    e2 = m.engine()
    assert e2.any_shape
    g = torch.Generator().manual_seed(6)
    pr, pc = torch.randn(33, 48, generator=g).cuda(), torch.randn(150, 48, generator=g).cuda()
    score = e2.score_all_pairs(pr, pc)
    for causal in (False, True):
        thr = _quantile(score, 0.9)
        _check(e2, pr, pc, thr, 4, 0, causal, score=score, what=("any-shape",))
        got = m.loop_closures_above(pr, pc, thr, window=4, causal=causal)
        _equal(got, _reference(score, thr, 4, 0, causal), "any-shape model")


def test_rows_above_on_a_strided_matrix(eng):
    rows, cols = _pooled(70, 1), _pooled(333, 2)
    big = torch.full((70, 400), float("nan"), device="cuda")
    view = big[:, 7:340]
    view.copy_(eng.score_all_pairs(rows, cols))
    assert view.stride(0) == 400
    thr = _quantile(view, 0.9)
    want = _reference(view.contiguous(), thr, 10, 5, False)
    _equal(eng.rows_above(view, thr, window=10, row0=5), want, "strided")
    _equal(eng.score_above(rows, cols, thr, window=10, row0=5), want, "fused")


def test_no_matrix_is_allocated(eng):
    n = 20000
    matrix = 4 * n * n
    assert eng.score_above_workspace_bytes(n, n) < 0.1 * matrix
    assert eng.score_above_workspace_bytes(300000, 300000) < 1e9
    pooled = _pooled(n, 11)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rows, cols, vals, rp = eng.score_above(pooled, pooled, 0.99, window=50, causal=True)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 0.1 * matrix
    assert rp.shape == (n + 1,) and int(rp[-1]) == rows.numel()
    assert rows.numel() == 0 or bool((cols < rows - 50).all())


def test_op_matches_engine(eng, kitti_pooled, ckpt_path):
    from sg_pr_amd import engine, ops  # noqa: F401
    from oracle import sgpr_oracle
    blob = torch.from_numpy(engine.blob_from_state_dict(sgpr_oracle.load_checkpoint(ckpt_path))).cuda()
    rows, cols = kitti_pooled[:300].contiguous(), kitti_pooled[:1500].contiguous()
    thr = 0.9
    want = eng.score_above(rows, cols, thr, window=10, causal=True)
    got = torch.ops.sgpr.score_above(rows, cols, blob, thr, 10, 0, True, None, None)
    _equal(got, want, "op")


def test_place_database_above(model):
    from sg_pr_amd import synth
    from sg_pr_amd.place_db import PlaceDatabase
    centers, labels, _, _ = synth.kitti_like_sequence(600, 100, seed=8)
    db = PlaceDatabase(model, capacity=16)
    db.add(centers, labels)
    eng = model.engine()
    ids = torch.arange(600)
    got = db.query_ids_above(ids, 0.9, window=10, causal=True)
    want = eng.score_above(db.pooled, db.pooled, 0.9, window=10, causal=True, row_self=ids.to(torch.int32))
    _equal(got, want, "query_ids_above")
    want_rows = eng.score_above(db.pooled, db.pooled, 0.9, window=10, causal=True)
    _equal(got, want_rows, "row_self = ids == row0 = 0")
    got = db.query_above(centers[:5], labels[:5], 0.8, window=-1)
    want = eng.score_above(model.embed(centers[:5], labels[:5])[0], db.pooled, 0.8, row0=600)
    _equal(got, want, "query_above")


def test_place_db_cli_threshold(model, tmp_path, ckpt_path):
    from sg_pr_amd import graph_store, metrics, place_db, synth
    centers, labels, _, poses = synth.kitti_like_sequence(500, 100, seed=12)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(500)])
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
    place_db.main([str(cfg), "--k", "2", "--window", "50"])
    assert not (tmp_path / "eva" / "07_above.npz").exists()            # without --threshold: nothing new
    place_db.main([str(cfg), "--k", "2", "--window", "50", "--threshold", "0.9", "--causal"])
    z = np.load(tmp_path / "eva" / "07_above.npz")
    rows, cols, scores = z["rows"], z["cols"], z["scores"]
    assert rows.shape == cols.shape == scores.shape and rows.dtype == np.int32
    assert np.all(scores >= np.float32(0.9)) and np.all(cols < rows - 50)
    order = rows.astype(np.int64) * 500 + cols
    assert np.all(np.diff(order) > 0)                                    # row-major, no repeats
    p, r = metrics.precision_recall_at(torch.from_numpy(rows), torch.from_numpy(cols), poses, p_thresh=3.0, window=50,
                                       causal=True)
    assert abs(float(z["precision"]) - p) < 1e-12 and abs(float(z["recall"]) - r) < 1e-12
    eng = model.engine()
    pooled = model.embed(centers, labels)[0]
    want = eng.score_above(pooled, pooled, 0.9, window=50, causal=True)
    assert rows.size == want[0].numel()


def _two_rank_worker(rank, world, port, ckpt, out_dir):
    import sys
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sg_pr_amd import allpairs, sg_net, synth
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt
    trainer = sg_net.SGTrainer(args, False)
    centers, labels, _, _ = synth.kitti_like_sequence(203, 100, 6)              # 102 + 101 rows: uneven shards
    dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
    scorer = allpairs.AllPairsScorer(model=trainer.model)
    for j, (thr, window, causal) in enumerate(((0.9, 5, False), (0.8, 0, True))):
        got = scorer.above(dc, dl, thr, window=window, causal=causal)
        if rank == 1:
            torch.save(tuple(t.cpu() for t in got), os.path.join(out_dir, "above_%d.pt" % j))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path, ckpt_path, model):
    import torch.multiprocessing as mp
    from sg_pr_amd import allpairs, synth
    mp.spawn(_two_rank_worker, args=(2, 29661, ckpt_path, str(tmp_path)), nprocs=2, join=True)
    centers, labels, _, _ = synth.kitti_like_sequence(203, 100, 6)
    scorer = allpairs.AllPairsScorer(model=model)
    for j, (thr, window, causal) in enumerate(((0.9, 5, False), (0.8, 0, True))):
        one = scorer.above(torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda(), thr, window=window,
                           causal=causal)
        two = torch.load(str(tmp_path / ("above_%d.pt" % j)))
        assert one[0].numel() > 0
        for a, b in zip(one, two):
            assert torch.equal(a.cpu(), b), j
