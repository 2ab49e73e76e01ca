"""sgpr_closure_consistency / sgpr_consistent_set on the MI355X against tests/consistency_ref.py, EQUAL to the bit: the
planted world in one group and in session groups, the word boundaries, decisions that sit exactly on a tolerance, void
closures, statelessness, the greedy clique on matrices it did not produce, SG.consistent_closures end to end and the
place_db command line."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consistency_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(max_trans=1.0, min_cos=math.cos(0.06), lever_gain=0.04)


def same(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def check(rows, cols, T, Xr, Xc, group, n_groups, max_trans=1.0, min_cos=math.cos(0.06), lever_gain=0.04):
    """both calls against the reference; -> the reference's (bool matrix, degree, members, rank, group_size)"""
    from sg_pr_amd import engine
    adj, degree, members = engine.closure_consistency(rows, cols, T, Xr, Xc, group, n_groups, max_trans, min_cos, lever_gain)
    rank, size = engine.consistent_set(adj, members, n_groups)
    torch.cuda.synchronize()
    w_adj, w_degree, w_members = ref.closure_consistency(rows, cols, T, Xr, Xc, group, n_groups, max_trans, min_cos,
                                                         lever_gain)
    w_rank, w_size = ref.consistent_set(w_adj, w_members, n_groups)
    assert same(adj, w_adj), "adjacency: %d words differ" % int((adj.cpu().numpy() != w_adj).sum())
    assert same(degree, w_degree) and same(members, w_members)
    assert same(rank, w_rank), (rank.cpu().numpy().tolist(), w_rank.tolist())
    assert same(size, w_size)
    return ref.unpack_bits(w_adj, len(w_degree)), w_degree, w_members, w_rank, w_size


@pytest.fixture(scope="module")
def world():
    from sg_pr_amd import synth
    return synth.closure_world(1, outlier_frac=0.5)


# ------------------------------------------------------------------ 1. the planted world
def test_world_one_group(world):
    w = world
    mat, degree, members, rank, size = check(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], np.zeros(400, np.int32), 1)
    sel = rank >= 0
    assert size[0] == sel.sum() >= 0.95 * w["planted"].sum() and not (sel & ~w["planted"]).any()


def test_world_session_groups(world):
    """3 x 2 session groups: group = row session x 2 + column session; closures are compared within a group only"""
    w = world
    group = (np.searchsorted([0, 200, 400], w["rows"], side="right") - 1) * 2 + (np.searchsorted([0, 300], w["cols"], side="right") - 1)
    mat, degree, members, rank, size = check(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], group.astype(np.int32), 6)
    assert len(np.unique(group)) >= 4 and not mat[group[:, None] != group[None, :]].any()
    assert size.sum() == (rank >= 0).sum() and (size > 0).sum() >= 4


@pytest.mark.parametrize("C", [0, 1, 2, 63, 64, 65, 129])
def test_word_boundaries(C):
    from sg_pr_amd import synth
    w = synth.closure_world(C, scans=80, closures=C, outlier_frac=0.3, alias=4)
    mat, degree, members, rank, size = check(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], np.zeros(C, np.int32), 1)
    assert size[0] == (rank >= 0).sum() and (C == 0 or size[0] >= 1)
    if C >= 63:
        assert degree.max() >= 0.5 * C                              # the planted set spans the words
    # ... and in two groups, which interleave inside every word
    check(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], (np.arange(C) % 2).astype(np.int32), 2)


# ------------------------------------------------------------------ 2. decisions exactly on a tolerance
EYE = [1.0, 0.0, 0.0, 0.0]


def _pair(Tp, Tq, Rq=(0.0, 0.0)):
    """two closures with identity rotations and integer translations: every product and sum is exact, and the residual
    is D.t = -T_q + T_p - R_p + R_q (columns at the origin, R_p at the origin)"""
    Xr = np.array([EYE, [1.0, 0.0, Rq[0], Rq[1]]])
    Xc = np.array([EYE])
    T = np.array([[1.0, 0.0, Tp[0], Tp[1]], [1.0, 0.0, Tq[0], Tq[1]]])
    return dict(rows=np.array([0, 1], np.int32), cols=np.zeros(2, np.int32), T=T, Xr=Xr, Xc=Xc, group=np.zeros(2, np.int32),
                n_groups=1)


def test_translation_boundary_is_inclusive():
    a = _pair((3.0, 4.0), (0.0, 0.0))                    # residual (3, 4): 25 <= 5 * 5
    assert check(**a, max_trans=5.0, min_cos=1.0, lever_gain=0.0)[1].tolist() == [1, 1]
    assert check(**a, max_trans=float(np.nextafter(5.0, 0.0)), min_cos=1.0, lever_gain=0.0)[1].tolist() == [0, 0]
    # the tolerance from the lever term alone: the row scans are (6, 8) apart, 0.5 x 10 = 5
    b = _pair((0.0, 0.0), (3.0, 4.0), Rq=(6.0, 8.0))     # residual -(3, 4) + (6, 8) = (3, 4)
    assert check(**b, max_trans=0.0, min_cos=1.0, lever_gain=0.5)[1].tolist() == [1, 1]
    assert check(**b, max_trans=0.0, min_cos=1.0, lever_gain=float(np.nextafter(0.5, 0.0)))[1].tolist() == [0, 0]
    assert check(**b, max_trans=0.0, min_cos=1.0, lever_gain=0.0)[1].tolist() == [0, 0]


def test_cosine_boundary_is_inclusive():
    from sg_pr_amd import synth
    w = synth.closure_world(7, scans=50, closures=2, outlier_frac=0.0, alias=0)
    G, H, R, _ = ref.prepare(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], np.zeros(2, np.int32), 1)
    dc = float(ref.compose(ref.compose(H[1], G[0]), R[1])[0])
    assert 0.99 < dc < 1.0                                # a genuine rotation: D.c is a rounded product sum
    args = (w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], np.zeros(2, np.int32), 1)
    assert check(*args, max_trans=1e6, min_cos=dc, lever_gain=0.0)[1].tolist() == [1, 1]
    assert check(*args, max_trans=1e6, min_cos=float(np.nextafter(dc, 2.0)), lever_gain=0.0)[1].tolist() == [0, 0]
    assert check(*args, max_trans=1e6, min_cos=float(np.nextafter(dc, 0.0)), lever_gain=0.0)[1].tolist() == [1, 1]
    assert check(*args, max_trans=1e6, min_cos=-math.inf, lever_gain=0.0)[1].tolist() == [1, 1]
    assert check(*args, max_trans=1e6, min_cos=math.inf, lever_gain=0.0)[1].tolist() == [0, 0]


# ------------------------------------------------------------------ 3. void closures
def test_void_closures_have_zero_rows_and_columns():
    from sg_pr_amd import synth
    w = synth.closure_world(5, scans=60, closures=70, outlier_frac=0.25, alias=0)
    C = 70
    rows, cols, T, group = w["rows"].copy(), w["cols"].copy(), w["T"].copy(), np.zeros(C, np.int32)
    rows[3], cols[5], rows[7], cols[9], group[11], group[13] = -1, -1, 60, 60, -1, 1
    T[15, 0], T[17, 3], T[66, 1] = np.nan, np.inf, -np.inf
    Xr, Xc = w["Xr"].copy(), w["Xc"].copy()
    Xr[rows[19], 2], Xc[cols[21], 1] = -np.inf, np.nan
    void = np.zeros(C, bool)
    void[[3, 5, 7, 9, 11, 13, 15, 17, 66]] = True
    void |= (rows == rows[19]) | (cols == cols[21])
    mat, degree, members, rank, size = check(rows, cols, T, Xr, Xc, group, 1)
    assert (members == np.where(void, -1, 0)).all()
    assert not mat[void].any() and not mat[:, void].any() and (degree[void] == 0).all() and (rank[void] == -1).all()
    clean = check(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], np.zeros(C, np.int32), 1)[0]
    keep = ~void
    assert (mat[np.ix_(keep, keep)] == clean[np.ix_(keep, keep)]).all() and size[0] > 10      # the neighbours are unaffected
    # empty pose tables: every closure is void
    e = np.zeros((0, 4))
    mat, degree, members, rank, size = check(w["rows"], w["cols"], w["T"], e, e, np.zeros(C, np.int32), 1)
    assert not mat.any() and (members == -1).all() and (rank == -1).all() and size.tolist() == [0]


# ------------------------------------------------------------------ 4. statelessness
def test_dirty_workspace_and_two_streams_give_equal_bytes(world):
    from sg_pr_amd import engine
    lib = engine.load_library()
    w = world
    C, W, ng = 400, 7, 6
    group = ((np.arange(C) * 7) % ng).astype(np.int32)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], group)]
    need_a, need_b = lib.sgpr_closure_consistency_workspace_bytes(C), lib.sgpr_consistent_set_workspace_bytes(C)
    outs = []
    torch.cuda.synchronize()
    for fill in (0xFF, 0x00):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            adj = torch.full((C, W), -1 if fill else 0, dtype=torch.int64, device="cuda")
            o32 = [torch.full((n,), 0x7f7f7f7f if fill else 0, dtype=torch.int32, device="cuda") for n in (C, C, ng)]
            ws_a = torch.full((need_a,), fill, dtype=torch.uint8, device="cuda")
            ws_b = torch.full((need_b,), fill, dtype=torch.uint8, device="cuda")
            st = ctypes.c_void_p(s.cuda_stream)
            rc = lib.sgpr_closure_consistency(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), C, dev[3].data_ptr(), 600,
                                              dev[4].data_ptr(), 600, dev[5].data_ptr(), ng, TOL["max_trans"], TOL["min_cos"],
                                              TOL["lever_gain"], adj.data_ptr(), o32[0].data_ptr(), ws_a.data_ptr(), need_a, st)
            assert rc == 0, lib.sgpr_last_error()
            rc = lib.sgpr_consistent_set(adj.data_ptr(), C, ws_a.data_ptr(), ng, o32[1].data_ptr(), o32[2].data_ptr(),
                                         ws_b.data_ptr(), need_b, st)
            assert rc == 0, lib.sgpr_last_error()
        outs.append((s, [adj, ws_a[:4 * C]] + o32))
    for s, _ in outs:
        s.synchronize()
    first, second = ([t.cpu().numpy().tobytes() for t in ts] for _, ts in outs)
    assert first == second
    w_adj, w_degree, w_members = ref.closure_consistency(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], group, ng, **TOL)
    w_rank, w_size = ref.consistent_set(w_adj, w_members, ng)
    assert first == [a.tobytes() for a in (w_adj, w_members, w_degree, w_rank, w_size)]


# ------------------------------------------------------------------ 5. the greedy clique on matrices it did not produce
def _random_symmetric(C, density, seed):
    rng = np.random.default_rng(seed)
    upper = np.triu(rng.random((C, C)) < density, 1)
    return upper | upper.T


@pytest.mark.parametrize("n_groups", [1, 7])
@pytest.mark.parametrize("density", [0.1, 0.9])
def test_consistent_set_on_random_symmetric_matrices(density, n_groups):
    from sg_pr_amd import engine
    C = 200
    rng = np.random.default_rng(int(density * 10) + n_groups)
    group = rng.integers(-1, n_groups + 1, size=C).astype(np.int32) if n_groups > 1 else np.zeros(C, np.int32)
    adj = ref.pack_bits(_random_symmetric(C, density, 11 * n_groups + int(density * 10)))
    rank, size = engine.consistent_set(torch.from_numpy(adj).cuda(), group, n_groups)
    w_rank, w_size = ref.consistent_set(adj, group, n_groups)
    assert same(rank, w_rank) and same(size, w_size)
    lit = ref.consistent_set_literal(adj, group, n_groups)
    assert (lit[0] == w_rank).all() and (lit[1] == w_size).all()
    assert size.sum().item() == (w_rank >= 0).sum() and w_size.max() >= 2


def test_consistent_set_ignores_junk_and_survives_asymmetry():
    from sg_pr_amd import engine
    C = 130                                               # three words, the last with 2 valid bits
    mat = _random_symmetric(C, 0.5, 3)
    group = (np.arange(C) % 3).astype(np.int32)
    clean = ref.consistent_set(ref.pack_bits(mat), group, 3)
    junk = ref.pack_bits(mat | np.eye(C, dtype=bool)).view(np.uint64).copy()
    junk[:, 2] |= np.uint64(0xfffffffffffffffc)           # bits 130..191 of every row
    rank, size = engine.consistent_set(torch.from_numpy(junk.view(np.int64)).cuda(), group, 3)
    assert same(rank, clean[0]) and same(size, clean[1])
    # not symmetric: rows decide, and the loop still ends
    rng = np.random.default_rng(4)
    lop = ref.pack_bits(rng.random((C, C)) < 0.5)
    rank, size = engine.consistent_set(torch.from_numpy(lop).cuda(), group, 3)
    want = ref.consistent_set_literal(lop, group, 3)
    assert same(rank, want[0]) and same(size, want[1])
    fast = ref.consistent_set(lop, group, 3)
    assert (fast[0] == want[0]).all()
    # the hand-made cases of the host test
    adj = ref.pack_bits(np.zeros((4, 4), bool))
    rank, size = engine.consistent_set(adj, np.zeros(4, np.int32), 2)
    assert rank.cpu().tolist() == [0, -1, -1, -1] and size.cpu().tolist() == [1, 0]


# ------------------------------------------------------------------ 6. end to end
@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_consistent_closures_end_to_end(model):
    """two 120-scan slices of one world as two sessions: the second re-drives the first; top-1 lists, verified, selected.
    The assertion is equality with the reference run on the verified records."""
    from sg_pr_amd import metrics, synth
    centers, labels, _, poses = synth.world_sequence(360, 100, seed=6)
    a, b = slice(0, 120), slice(240, 360)                 # the map session and the session that revisits it
    pooled = model.embed(centers, labels)[0]
    model.engine().check_status()
    vals, idx = model.loop_closures(pooled[b], pooled[a], k=1)
    ver = model.verify_closures(centers[b], labels[b], idx, values=vals, min_inliers=12, col_centers=centers[a],
                                col_labels=labels[a])
    rows = np.arange(120, dtype=np.int64)[:, None]
    # the map session's odometry lives in a frame of its own
    frame = np.array([math.cos(2.3), math.sin(2.3), -310.0, 95.0])
    Xr, Xc = metrics.planar_odometry(poses[b]), ref.compose(frame, metrics.planar_odometry(poses[a]))
    host = {k: ver[k].cpu().numpy() for k in ("refined", "flags", "accept")}
    cols = idx.cpu().numpy()
    for row_sessions, kw in ((None, {}), ([0, 50], dict(max_trans=0.8, max_yaw=0.05, lever_gain=0.03, min_clique=40))):
        out = model.consistent_closures(ver, rows, idx, Xr, col_poses=Xc, row_sessions=row_sessions, **kw)
        torch.cuda.synchronize()
        want = ref.consistent_closures(host["refined"].reshape(-1, 4), host["flags"], host["accept"], rows, cols, Xr, Xc,
                                       row_starts=row_sessions, **kw)
        for name in ("accept", "rank", "degree"):
            assert out[name].shape == (120, 1) and same(out[name].reshape(-1), want[name]), name
        assert same(out["group_size"], want["group_size"])
        assert not (out["accept"].cpu().numpy() & ~host["accept"]).any()
    # poses as KITTI rows work alike (one frame for both sessions)
    out = model.consistent_closures(ver, rows, idx, poses[b], col_poses=poses[a])
    want = ref.consistent_closures(host["refined"].reshape(-1, 4), host["flags"], host["accept"], rows, cols,
                                   metrics.planar_odometry(poses[b]), metrics.planar_odometry(poses[a]))
    assert same(out["accept"].reshape(-1), want["accept"]) and same(out["group_size"], want["group_size"])
    assert want["group_size"][0] >= 3 and want["accept"].sum() == want["group_size"][0]


def test_place_db_consistent_cli(model, tmp_path, ckpt_path, capsys):
    """--verify --consistent: the file holds the closures that entered and the selection is the reference's on them"""
    from sg_pr_amd import graph_store, metrics, place_db, synth
    centers, labels, _, poses = synth.world_sequence(150, 100, seed=4)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(150)])
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
    place_db.main([str(cfg), "--k", "2", "--window", "30", "--verify", "--min-inliers", "15", "--consistent", "--sessions", "2",
                   "--max-trans", "0.8", "--max-yaw-deg", "3", "--lever-gain", "0.03", "--min-clique", "4"])
    line = next(l for l in capsys.readouterr().out.splitlines() if "pairwise consistent" in l)
    z = np.load(tmp_path / "eva" / "07_consistent.npz")
    ver = np.load(tmp_path / "eva" / "07_verify.npz")
    assert z["session_starts"].tolist() == [0, 75] and z["group_size"].shape == (4,)
    n = int(ver["accept"].sum())
    assert z["accepted"] == n == z["rows"].size and z["refined"].shape == (n, 4) and "accepted %d " % n in line
    X = metrics.planar_odometry(poses)
    want = ref.consistent_closures(z["refined"], np.zeros(n, np.int32), None, z["rows"], z["cols"], X, X, row_starts=[0, 75],
                                   col_starts=[0, 75], max_trans=0.8, max_yaw=math.radians(3.0), lever_gain=0.03, min_clique=4)
    assert np.array_equal(z["consistent"], want["accept"]) and np.array_equal(z["rank"], want["rank"])
    assert np.array_equal(z["degree"], want["degree"]) and np.array_equal(z["group_size"], want["group_size"])
    assert z["consistent_count"] == want["accept"].sum() and "consistent %d " % want["accept"].sum() in line
    assert 0.0 <= z["precision_accepted"] <= 1.0 and 0.0 <= z["precision_consistent"] <= 1.0
