"""sgpr_topk_rows_large / sgpr_score_topk_large: loop-closure lists for k up to 4096.  The resident form against the masked
stable sort of the matrix (values as bit patterns, indices exactly), the pooled form against the same handle's
score_all_pairs on the same rectangle plus that sort, agreement with the k <= 16 entry points, dirty workspaces, the
routing of Engine.score_topk / topk_rows and the place_db CLI's recall@1 %."""
import os

import numpy as np
import pytest
import torch

import score_ref
from test_gpu_row_blocks import M_A, RB_A, SHAPES, _rb, _rows_quantity, _scale_row
from test_gpu_score_range import _any_shape, _wide_checkpoint
from test_gpu_stateless import _check_all_patterns
from test_gpu_topk import _reference

pytestmark = pytest.mark.gpu

KS = (1, 3, 16, 17, 45, 100, 1000, 4096)


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
def kitti_pooled(eng):
    from sg_pr_amd import synth
    centers, labels, _, _ = synth.kitti_like_sequence(4541, 100, seed=3)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    return pooled


def _equal(got, want, what):
    gv, gi = got
    wv, wi = want
    assert gv.shape == wv.shape and gi.shape == wi.shape, (what, gv.shape, wv.shape)
    bad = (gv.view(torch.int32) != wv.view(torch.int32)) | (gi != wi)
    assert not bad.any(), (what, bad.nonzero()[:5].tolist(), int(bad.sum()))


def _scores(r, m, seed, ld=None):
    """SG-PR-like rows (most scores within 1e-3 of 1, a long tail below) with planted ties around the top, -0.0 next to
    +0.0, subnormals, +-inf and NaN; ld > m gives a strided view"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ld = ld or m
    s = 1.0 - torch.exp(torch.randn(r, ld, generator=g, device="cuda") * 2.0 - 6.0)
    s = torch.where(torch.rand(r, ld, generator=g, device="cuda") < 0.15, torch.rand(r, ld, generator=g, device="cuda"), s)
    q = torch.rand(r, ld, generator=g, device="cuda") < 0.3                  # quantised entries: many exact ties
    s = torch.where(q, torch.round(s * 4096.0) / 4096.0, s).float()
    n = r * ld
    flat = s.view(-1)
    for val, frac in ((0.0, 0.002), (-0.0, 0.002), (1e-40, 0.001), (-1e-40, 0.001), (float("inf"), 0.0005),
                      (-float("inf"), 0.001), (float("nan"), 0.002), (-5.0, 0.001)):
        pos = torch.randint(0, n, (max(1, int(n * frac)),), generator=g, device="cuda")
        flat[pos] = val
    return s[:, :m]


def _ref(score, k, window=-1, row0=0, causal=False, row_self=None):
    """test_gpu_topk._reference with -0.0 sorted as +0.0 (whatever the device sort makes of the sign bit) and every value
    read back from the matrix at its index: the stored bits"""
    score = score.contiguous()
    _, i = _reference(score + 0.0, k, window=window, row0=row0, causal=causal, row_self=row_self)
    i = i.contiguous()
    v = torch.full(i.shape, -float("inf"), device=score.device)
    ok = i >= 0
    if score.shape[1]:
        v[ok] = score.gather(1, i.clamp(min=0).long())[ok]
    return v, i


def _rows_to_reference(score, kmax, window=-1, row0=0, causal=False, row_self=None):
    return _ref(score, kmax, window=window, row0=row0, causal=causal, row_self=row_self)


def _check_resident(eng, score, ks, modes, what, row0=0):
    r, m = score.shape
    for window, causal, row_self in modes:
        kmax = max(ks)
        wv, wi = _rows_to_reference(score, kmax, window=window, row0=row0, causal=causal, row_self=row_self)
        for k in ks:
            got = eng.topk_rows_large(score, k=k, row0=row0, window=window, causal=causal, row_self=row_self)
            _equal(got, (wv[:, :k].contiguous(), wi[:, :k].contiguous()), (what, r, m, k, window, causal,
                                                                            row_self is not None))


def _modes(r, m, seed):
    perm = torch.from_numpy(np.random.default_rng(seed).integers(0, max(m, 1), size=r).astype(np.int32))
    return [(-1, False, None), (0, False, None), (50, False, None), (50, True, None), (-1, True, None),
            (10, False, perm), (10, True, perm)]


# ------------------------------------------------------------------------------------------------- resident form
@pytest.mark.parametrize("shape", [(1, 1), (37, 131), (300, 517)])
def test_resident_small_shapes(eng, shape):
    r, m = shape
    score = _scores(r, m, r + m)
    _check_resident(eng, score, KS + (m + 5,), _modes(r, m, 1), "small")
    # ld > M (and a row start that is not 16-byte aligned: ld odd)
    wide = _scores(r, m, r + m + 1, ld=m + 3)
    _check_resident(eng, wide, (1, 17, 100, m + 1), _modes(r, m, 2)[:3], "ld > M")


def test_resident_kitti_square(eng):
    score = _scores(4541, 4541, 7)
    _check_resident(eng, score, KS, _modes(4541, 4541, 3), "4541^2")


@pytest.mark.parametrize("shape", [(3, 262144), (1, 1048576)])
def test_resident_long_rows(eng, shape):
    r, m = shape
    score = _scores(r, m, 11)
    # ties that straddle the chunk boundaries of a split row: equal values on both sides of every 1024 / 4096 column
    # edge, and at the k-th value of the row
    edges = torch.arange(1024, m, 1024, device="cuda")
    for d in (-2, -1, 0, 1):
        score[:, (edges + d).clamp(0, m - 1)] = 0.99951171875
    _check_resident(eng, score, KS, _modes(r, m, 4)[:5], "long")
    kth = _rows_to_reference(score, 1000)[0][:, 999:1000]                 # the 1000th value planted 3000 times more
    idx = torch.randint(0, m, (r, 3000), device="cuda")
    score.scatter_(1, idx, kth.expand(r, 3000).contiguous())
    _check_resident(eng, score, (999, 1000, 1001, 4096), [(-1, False, None), (50, True, None)], "long, planted k-th")


def test_rows_with_fewer_eligible_columns_than_k(eng):
    score = _scores(20, 300, 5)
    score[3] = float("nan")
    score[4] = -float("inf")
    score[5, 100:] = -float("inf")
    _check_resident(eng, score, (1, 17, 290, 299, 300, 301, 4096), _modes(20, 300, 6), "short rows")
    v, i = eng.topk_rows_large(score, k=4096, window=50)
    assert (i[3] == -1).all() and (v[3] == -float("inf")).all()
    # the same from pooled vectors: the NaN graphs really are NaN in the matrix, and absent from the lists
    rows, cols = _pooled(40, 32, 3.0, 5), _pooled(300, 32, 3.0, 6)
    cols[250] = float("nan")
    rows[3] = float("nan")
    pscore = eng.score_all_pairs(rows, cols)
    assert torch.isnan(pscore[3]).all() and torch.isnan(pscore[:, 250]).all()
    for k in (17, 300):
        v, i = eng.score_topk_large(rows, cols, k=k)
        assert (i[3] == -1).all() and (v[3] == -float("inf")).all()
        assert (i != 250).all()
    # no column at all
    v, i = eng.topk_rows_large(torch.empty(3, 0, device="cuda"), k=20)
    assert (i == -1).all() and (v == -float("inf")).all()


# ------------------------------------------------------------------------------------------------- pooled form
def _pooled(n, width, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, width, generator=g) * scale).cuda()


def _check_pooled(e, rows, cols, cases, what):
    score = e.score_all_pairs(rows, cols)
    for k, window, row0, causal, row_self in cases:
        got = e.score_topk_large(rows, cols, k=k, window=window, row0=row0, causal=causal, row_self=row_self)
        want = _ref(score, k, window=window, row0=row0, causal=causal, row_self=row_self)
        _equal(got, want, (what, rows.shape[0], cols.shape[0], k, window, row0, causal))
    return score


def test_pooled_kitti_production(eng, kitti_pooled):
    cases = [(45, 50, 0, False, None), (45, 50, 0, True, None), (1000, 50, 0, True, None), (4096, -1, 0, False, None)]
    _check_pooled(eng, kitti_pooled, kitti_pooled, cases, "production, KITTI-like")


def test_pooled_kitti_fallback_handles(eng, sd, kitti_pooled):
    from sg_pr_amd import engine
    wide = engine.Engine(_wide_checkpoint(sd), device=0)
    try:
        assert not wide.uses_f16_planes()
        cases = [(45, 50, 0, False, None), (45, 50, 0, True, None)]
        _check_pooled(wide, kitti_pooled, kitti_pooled, cases, "wide checkpoint, KITTI-like")
    finally:
        wide.close()
    eng.set_skip_mask(1 << 13)
    try:
        _check_pooled(eng, kitti_pooled[:900].contiguous(), kitti_pooled, [(45, 50, 0, True, None)], "bit 13")
    finally:
        eng.set_skip_mask(0)
    any_eng = _any_shape(_any_shape())
    try:
        rows = _pooled(4541, 48, 1.0, 21)
        _check_pooled(any_eng, rows, rows, [(45, 50, 0, False, None), (45, 50, 0, True, None)], "any-shape, KITTI-like")
    finally:
        any_eng.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_pooled_several_blocks(eng, sd, shape):
    from sg_pr_amd import engine
    m, r = shape
    rb = _rb(r, m)
    assert rb < r                                                       # more than one 64 MB block runs
    assert eng.score_topk_large_workspace_bytes(r, m, 100) < 4 * r * m or r < 2 * rb
    perm = torch.from_numpy(np.random.default_rng(r).integers(0, m, size=r).astype(np.int32))
    cases = [(100, 50, 0, False, None), (45, 5, 7, True, None), (17, 10, 0, True, perm)]
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    _check_pooled(eng, rows, cols, cases, ("production", shape))
    wide = engine.Engine(_wide_checkpoint(sd), device=0)
    try:
        _check_pooled(wide, rows, cols, cases[:1], ("wide checkpoint", shape))
    finally:
        wide.close()
    any_eng = _any_shape(_any_shape())
    try:
        ar, ac = _pooled(r, 48, 1.0, r + 1), _pooled(m, 48, 1.0, m + 1)
        _check_pooled(any_eng, ar, ac, cases[:2], ("any-shape", shape))
    finally:
        any_eng.close()


def test_pooled_one_query_long_map(eng):
    rows, cols = _pooled(1, 32, 3.0, 1), _pooled(262144, 32, 3.0, 2)
    _check_pooled(eng, rows, cols, [(4096, -1, 262143, True, None), (4096, 50, 0, False, None), (1000, 50, 200000, True,
                                                                                                  None)], "one query")


@pytest.mark.parametrize("where", ["first", "last"])
def test_mixed_range_production_handle(eng, sd, where):
    """One row beyond the exact-path gate in the first or the last 64 MB block: every block takes the datapath
    score_all_pairs takes on the whole rectangle (the call's f16 range is answered once)."""
    m = 300
    rb = _rb(1 << 30, m)
    r = rb + 37
    rows, cols = _pooled(r, 32, 1.0, 41), _pooled(m, 32, 1.0, 42)
    rn, cn = rows.cpu().numpy(), cols.cpu().numpy()
    thr = score_ref.F16_SAFE
    assert _rows_quantity(sd, rn, cn, "bound", score_ref.TUNED_K) < 0.97 * thr
    where_i = 5 if where == "first" else r - 3
    s = _scale_row(sd, rn[where_i:where_i + 1], cn, "bound", 1.03 * thr, score_ref.TUNED_K)
    rows[where_i] *= s
    score = eng.score_all_pairs(rows, cols)
    b0 = 0 if where_i >= rb else rb
    alone = eng.score_all_pairs(rows[b0:b0 + rb].contiguous(), cols)
    assert int((alone.view(torch.int32) != score[b0:b0 + rb].view(torch.int32)).sum()) > 0   # the case can tell
    for k, window, causal in ((17, -1, False), (100, 5, True)):
        got = eng.score_topk_large(rows, cols, k=k, window=window, row0=5, causal=causal)
        _equal(got, _ref(score, k, window=window, row0=5, causal=causal), ("mixed", where, k))


# ------------------------------------------------------------------------------------------------- k <= 16
def test_large_paths_equal_the_k16_paths(eng, kitti_pooled):
    rows, cols = kitti_pooled[:700].contiguous(), kitti_pooled
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(9).permutation(4541)[:700].astype(np.int32))
    for k in (1, 4, 8, 16):
        for window, causal, row_self in ((-1, False, None), (50, False, None), (50, True, None), (20, False, perm),
                                         (20, True, perm)):
            want = eng.score_topk(rows, cols, k=k, window=window, row0=3, causal=causal, row_self=row_self)
            got = eng.score_topk_large(rows, cols, k=k, window=window, row0=3, causal=causal, row_self=row_self)
            _equal(got, want, ("score_topk", k, window, causal))
            got_r = eng.topk_rows_large(score, k=k, row0=3, window=window, causal=causal, row_self=row_self)
            _equal(got_r, want, ("topk_rows_large", k, window, causal))
        for window in (-1, 0, 50):
            want = eng.topk_rows(score, k=k, row0=3, window=window)     # sgpr_topk_rows
            _equal(eng.topk_rows_large(score, k=k, row0=3, window=window), want, ("topk_rows", k, window))
    eng.check_status()


# ------------------------------------------------------------------------------------------------- statelessness
def test_dirty_workspaces_and_status(eng, kitti_pooled):
    from sg_pr_amd.engine import SgprError
    rows, cols = kitti_pooled[:300].contiguous(), kitti_pooled
    score = _scores(300, 4541, 13)
    _check_all_patterns(eng, lambda: eng.score_topk_large(rows, cols, k=100, window=50, causal=True), "score_topk_large")
    _check_all_patterns(eng, lambda: eng.topk_rows_large(score, k=1000, window=50), "topk_rows_large")
    _check_all_patterns(eng, lambda: eng.topk_rows_large(score[:1], k=4096), "topk_rows_large, one row")
    bad = torch.tensor([0, 3, 4541, 1], dtype=torch.int32)
    eng.topk_rows_large(score[:4], k=30, row_self=bad)
    with pytest.raises(SgprError, match="row_self"):
        eng.check_status()
    eng.score_topk_large(rows[:4].contiguous(), cols, k=30, row_self=bad)
    with pytest.raises(SgprError, match="row_self"):
        eng.check_status()
    eng.check_status()


# ------------------------------------------------------------------------------------------------- routing, CLI
@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_routing_and_place_database(eng, kitti_pooled, model):
    from sg_pr_amd import synth
    from sg_pr_amd.place_db import PlaceDatabase
    rows = kitti_pooled[:50].contiguous()
    _equal(eng.score_topk(rows, kitti_pooled, k=100, window=50), eng.score_topk_large(rows, kitti_pooled, k=100, window=50),
           "score_topk k=100")
    score = eng.score_all_pairs(rows, kitti_pooled)
    _equal(eng.topk_rows(score, k=45, window=50), eng.topk_rows_large(score, k=45, window=50), "topk_rows k=45")
    _equal(eng.topk_rows(score, k=4, window=50, causal=True), _ref(score, 4, window=50, causal=True), "causal k=4")
    centers, labels, _, _ = synth.kitti_like_sequence(400, 100, seed=8)
    db = PlaceDatabase(model, capacity=16)
    db.add(centers, labels)
    v, i = db.query_ids(range(400), k=100, window=10)
    _equal((v, i), _ref(model.engine().score_all_pairs(db.pooled, db.pooled), 100, window=10), "query_ids k=100")
    qv, qi = db.query(centers[:3], labels[:3], k=300)
    assert qv.shape == (3, 300) and (qi >= 0).all()
    mv, mi = model.loop_closures(db.pooled[:5], db.pooled, k=64, window=10, row0=0)
    _equal((mv, mi), (v[:5, :64].contiguous(), i[:5, :64].contiguous()), "loop_closures k=64")
    from sg_pr_amd import engine, ops  # noqa: F401
    blob = torch.from_numpy(engine.blob_from_state_dict(model.state_dict())).cuda()
    ov, oi = torch.ops.sgpr.score_topk(db.pooled[:5].contiguous(), db.pooled, blob, 64, 10, 0, False, None)
    _equal((ov, oi), (mv, mi), "torch.ops.sgpr.score_topk k=64")


def test_place_db_cli_recall_percent(model, tmp_path, ckpt_path):
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
    place_db.main([str(cfg), "--k", "2", "--window", "50", "--recall-percent", "1"])
    z = np.load(tmp_path / "eva" / "07_topk.npz")
    assert int(z["recall_percent_n"]) == 5 and z["indices"].shape == (500, 5)
    want, n = metrics.recall_at_percent(torch.from_numpy(z["indices"]), poses, percent=1.0, p_thresh=3.0, window=50)
    assert n == 5 and float(z["recall_percent"]) == want
    place_db.main([str(cfg), "--k", "20", "--window", "50", "--recall-percent", "1"])   # k = max(--k, N)
    z = np.load(tmp_path / "eva" / "07_topk.npz")
    assert z["indices"].shape == (500, 20) and int(z["recall_percent_n"]) == 5
    place_db.main([str(cfg), "--k", "4", "--window", "50"])                            # without the flag: as before
    z = np.load(tmp_path / "eva" / "07_topk.npz")
    assert sorted(z.files) == ["frame", "indices", "recall", "scores"]
