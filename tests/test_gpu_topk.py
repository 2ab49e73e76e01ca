"""sgpr_score_topk: loop-closure candidates straight from pooled vectors (fused score + top-k, no matrix), its causal rule,
the handles without a fused instance, the place database and its CLI - every value against the matrix path's bits."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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
    centers, labels, _, poses = synth.kitti_like_sequence(4541, 100, seed=3)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    return pooled


def _pooled(n, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 32, generator=g) * scale).cuda()


def _reference(score, k, window=-1, row0=0, causal=False, row_self=None):
    """Stable descending sort of the dense matrix after masking the ineligible columns (and NaN) -> (values, indices)."""
    r, m = score.shape
    s = score.clone()
    s[torch.isnan(s)] = -float("inf")
    self_ = (torch.arange(r, device=s.device) + row0) if row_self is None else row_self.to(s.device).long()
    c = torch.arange(m, device=s.device)
    bad = torch.zeros_like(s, dtype=torch.bool)
    if window >= 0:
        bad |= (c[None, :] - self_[:, None]).abs() <= window
    if causal:
        bad |= c[None, :] >= self_[:, None]
    s[bad] = -float("inf")
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    v, i = v[:, :k], i[:, :k].to(torch.int32)
    if v.shape[1] < k:
        pad = k - v.shape[1]
        v = torch.cat((v, torch.full((r, pad), -float("inf"), device=v.device)), dim=1)
        i = torch.cat((i, torch.full((r, pad), -1, dtype=torch.int32, device=i.device)), dim=1)
    i[v == -float("inf")] = -1
    return v, i


def _check_against_topk_rows(eng, rows, cols, k, window, row0):
    score = eng.score_all_pairs(rows, cols)
    kk = 4 if k == 3 else k
    want_v, want_i = eng.topk_rows(score, k=kk, row0=row0, window=window)
    got_v, got_i = eng.score_topk(rows, cols, k=k, window=window, row0=row0)
    assert got_v.shape == (rows.shape[0], k)
    assert torch.equal(got_v, want_v[:, :k].contiguous()), (rows.shape[0], cols.shape[0], k, window, row0)
    assert np.array_equal(got_i.cpu().numpy(), want_i[:, :k].cpu().numpy()), (rows.shape[0], cols.shape[0], k, window, row0)


@pytest.mark.parametrize("shape", [(37, 131), (1, 4541), (300, 517)])
def test_fused_topk_equals_matrix_plus_topk_rows(eng, shape):
    r, m = shape
    rows, cols = _pooled(r, r), _pooled(m, m + 1)
    for k in (1, 3, 4, 8, 16):
        for window in (-1, 0, 10, 50):
            for row0 in (0, 120):
                _check_against_topk_rows(eng, rows, cols, k, window, row0)


def test_fused_topk_full_kitti_like_set(eng, kitti_pooled):
    for k in (1, 3, 16):
        for window in (-1, 50):
            _check_against_topk_rows(eng, kitti_pooled, kitti_pooled, k, window, 0)


def test_ties_nan_and_short_rows(eng):
    rows, cols = _pooled(40, 5), _pooled(300, 6)
    cols[100:140] = cols[7]                      # 41 equal columns: exact ties, the lowest column wins
    cols[250] = float("nan")
    rows[3] = float("nan")
    for k in (1, 4, 16):
        _check_against_topk_rows(eng, rows, cols, k, -1, 0)
        _check_against_topk_rows(eng, rows, cols, k, 10, 0)
        v, i = eng.score_topk(rows, cols, k=k)
        score = eng.score_all_pairs(rows, cols)
        got = score.gather(1, i.clamp(min=0).long())
        assert not torch.isnan(v).any() and not torch.isnan(got[i >= 0]).any()   # a NaN score ranks last: never reported
        assert torch.equal(got[i >= 0], v[i >= 0])
        # the NaN graphs really are NaN in the matrix (not scored like a healthy graph upstream), and absent from the lists
        assert torch.isnan(score[3]).all() and torch.isnan(score[:, 250]).all()
        assert (i[3] == -1).all() and (v[3] == -float("inf")).all()
        assert (i != 250).all()
    # fewer than k eligible columns -> (-inf, -1) in the remaining slots
    few = _pooled(6, 9)
    for k in (4, 16):
        _check_against_topk_rows(eng, rows[:6].contiguous(), few, k, 2, 0)
        v, i = eng.score_topk(rows[:6].contiguous(), few, k=k, window=2, causal=True)
        assert (i[0] == -1).all() and (i[:, 5:] == -1).all()
    v, i = eng.score_topk(rows[:3].contiguous(), cols[:0], k=4)              # no column at all
    assert (i == -1).all() and (v == -float("inf")).all()


def test_causal_equals_masked_stable_sort(eng, kitti_pooled):
    rows = kitti_pooled[:700].contiguous()
    for m in (700, 4541):
        cols = kitti_pooled[:m].contiguous()
        score = eng.score_all_pairs(rows, cols)
        for k in (1, 5, 16):
            for window in (-1, 0, 50):
                for row0 in (0, 37):
                    got = eng.score_topk(rows, cols, k=k, window=window, row0=row0, causal=True)
                    want = _reference(score, k, window=window, row0=row0, causal=True)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (m, k, window, row0)
        perm = torch.from_numpy(np.random.default_rng(m).permutation(m)[:700].astype(np.int32))
        for causal in (False, True):
            got = eng.score_topk(rows, cols, k=8, window=20, causal=causal, row_self=perm)
            want = _reference(score, 8, window=20, causal=causal, row_self=perm)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (m, causal)
    eng.check_status()


def test_row_self_out_of_range_is_reported(eng):
    from sg_pr_amd.engine import SgprError
    rows, cols = _pooled(4, 1), _pooled(50, 2)
    eng.score_topk(rows, cols, k=1, row_self=torch.tensor([0, 3, 50, 1], dtype=torch.int32))
    with pytest.raises(SgprError, match="row_self"):
        eng.check_status()
    eng.check_status()                                                    # the report was consumed


def test_range_guard_and_both_modes(eng, kitti_pooled):
    """x 1000: the exact fp32 per-pair path (slow_tile); x 0.25 / x 2: both forms of the f16 path - same bits as the matrix."""
    for scale, r, m in ((1000.0, 19, 300), (0.25, 300, 1200), (2.0, 300, 1200)):
        rows = (kitti_pooled[:r] * scale).contiguous()
        cols = (kitti_pooled[1000:1000 + m] * scale).contiguous()
        score = eng.score_all_pairs(rows, cols)
        for k in (1, 4, 16):
            for causal in (False, True):
                got = eng.score_topk(rows, cols, k=k, window=5, row0=3, causal=causal)
                want = _reference(score, k, window=5, row0=3, causal=causal)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (scale, k, causal)


def test_fallback_handles(eng, kitti_pooled):
    """The wide-range instance (debug bit 13) and an any-shape handle: bit-equal to their own matrix + top-k."""
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    rows, cols = kitti_pooled[:200].contiguous(), kitti_pooled[:900].contiguous()
    eng.set_skip_mask(1 << 13)
    try:
        score = eng.score_all_pairs(rows, cols)
        for k, causal in ((1, False), (4, True), (16, False)):
            got = eng.score_topk(rows, cols, k=k, window=10, causal=causal)
            want = _reference(score, k, window=10, causal=causal)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ("wide", k, causal)
    finally:
        eng.set_skip_mask(0)
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
    for k, causal in ((1, False), (3, True), (16, False)):
        got = m.loop_closures(pr, pc, k=k, window=4, causal=causal)
        want = _reference(score, k, window=4, causal=causal)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ("any-shape", k, causal)


def test_no_matrix_is_allocated(eng):
    n = 20000
    matrix = 4 * n * n
    for k in (1, 16):
        ws = eng.score_topk_workspace_bytes(n, n, k)
        allpairs = int(eng.lib.sgpr_score_all_pairs_workspace_bytes(eng._h, n, n))
        grid = eng.num_cus * 4
        assert ws < 0.1 * matrix
        assert ws <= allpairs + (n + 16 * grid) * k * 8 + 4096, (ws, allpairs)
    pooled = _pooled(n, 11)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v, i = eng.score_topk(pooled, pooled, k=16, window=50, causal=True)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 0.1 * matrix
    assert v.shape == (n, 16) and int(i[0, 0]) == -1 and int(i[-1, 0]) >= 0


def test_place_database(model, tmp_path, ckpt_path):
    from sg_pr_amd import synth
    from sg_pr_amd.place_db import PlaceDatabase
    centers, labels, _, _ = synth.kitti_like_sequence(600, 100, seed=8)
    db = PlaceDatabase(model, capacity=16)
    cuts = [0, 150, 151, 600]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ids = db.add(centers[a:b], labels[a:b])
        assert ids.tolist() == list(range(a, b))
        assert torch.equal(db.pooled[a:b], model.embed(centers[a:b], labels[a:b])[0])
    one = model.embed(centers, labels)[0]
    assert len(db) == 600 and float((db.pooled - one).abs().max()) <= 1e-5
    # members, causal == frame t asked online against the first t frames
    v, i = db.query_ids(range(600), k=4, window=10, causal=True)
    eng = model.engine()
    for t in range(600):
        ov, oi = eng.score_topk(db.pooled[t:t + 1], db.pooled[:t], k=4, window=10, row0=t, causal=True)
        assert torch.equal(ov[0], v[t]) and torch.equal(oi[0], i[t]), t
    # graphs that are not members: frames len(db), len(db) + 1, ...
    qv, qi = db.query(centers[:5], labels[:5], k=2, window=-1)
    wv, wi = eng.score_topk(model.embed(centers[:5], labels[:5])[0], db.pooled, k=2, row0=600)
    assert torch.equal(qv, wv) and torch.equal(qi, wi)
    # save / load round trip; another checkpoint is refused
    path = str(tmp_path / "db.npz")
    db.save(path)
    back = PlaceDatabase.load(path, model)
    assert torch.equal(back.pooled, db.pooled)
    bv, bi = back.query_ids(range(600), k=4, window=10, causal=True)
    assert torch.equal(bv, v) and torch.equal(bi, i)
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    other = sg_net.SGTrainer(args, False).model.eval()
    with torch.no_grad():
        other.scoring_layer.bias.add_(0.5)
    with pytest.raises(ValueError, match="checkpoint"):
        PlaceDatabase.load(path, other)


def test_place_db_cli_matches_evaluate_all_pairs(model, tmp_path, ckpt_path, golden_dir):
    from sg_pr_amd import graph_store, place_db, synth
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
    res = place_db.main([str(cfg), "--k", "4", "--window", "50"])
    z = np.load(tmp_path / "eva" / "07_topk.npz")
    assert z["indices"].shape == (500, 4) and z["scores"].shape == (500, 4)
    assert np.array_equal(z["frame"], np.arange(500))
    ref = graph_store.evaluate_all_pairs(model, seq, top_k=1, window=50)
    assert np.array_equal(z["indices"][:, 0], ref["closure_frames"][:, 0].cpu().numpy())
    assert np.array_equal(z["scores"][:, 0], ref["closure_scores"][:, 0].cpu().numpy())
    assert res["07"].shape == (4,) and np.all(np.diff(res["07"]) >= 0)
