"""sgpr_localize_scans on the MI355X against tests/localize_ref.py, EQUAL to the bit in pose, stat and spread (NaN
compared as NaN): the planted world with and without odometry, slot counts at every block-size boundary, session tables,
empty maps, padding and accept masks, non-finite inputs in every array, decisions exactly at a tolerance, duplicated and
degenerate hypotheses, outputs pre-filled with 0xFF on two streams, SG.localize end to end and the place_db command line."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localize_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
MIN_COS = math.cos(0.1)
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


def same(got, want):
    """equal to the bit, NaN (of any payload) compared as NaN"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return got.tobytes() == want.tobytes()
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all()) and np.where(gn, 0.0, got).tobytes() == np.where(wn, 0.0, want).tobytes()


def raw(map_poses, cols, T, accept=None, odo=None, starts=None, L=1, max_trans=1.0, min_cos=MIN_COS, stream=None):
    """the C call on host arrays, every output byte pre-filled with 0xFF -> (pose, stat, spread) device tensors"""
    from sg_pr_amd import engine, localize
    lib = localize.load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    cols = np.asarray(cols, np.int32)
    Q, K = cols.shape
    m = np.asarray(map_poses, np.float64).reshape(-1, 4)
    d_map = torch.as_tensor(m if m.shape[0] else np.zeros((1, 4)), device=dev)
    d_cols = torch.as_tensor(cols, device=dev)
    d_T = torch.as_tensor(np.ascontiguousarray(np.asarray(T, np.float64).reshape(Q, K, 4)), device=dev)
    d_acc = None if accept is None else torch.as_tensor(np.asarray(accept, np.uint8).reshape(Q, K), device=dev)
    d_odo = None if odo is None else torch.as_tensor(np.asarray(odo, np.float64).reshape(Q, 4), device=dev)
    table = None if starts is None else np.ascontiguousarray(np.asarray(starts, np.int32))
    pose = torch.full((Q * 32,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float64).view(Q, 4)
    stat = torch.full((Q * 16,), 0xFF, dtype=torch.uint8, device=dev).view(torch.int32).view(Q, 4)
    spread = torch.full((Q * 8,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float64)
    s = torch.cuda.current_stream() if stream is None else stream
    s.wait_stream(torch.cuda.current_stream())
    rc = lib.sgpr_localize_scans(engine._ptr(d_map), m.shape[0], engine._ptr(d_cols), engine._ptr(d_T), engine._ptr(d_acc),
                                 Q, K, engine._ptr(d_odo), None if table is None else table.ctypes.data,
                                 0 if table is None else table.size, L, float(max_trans), float(min_cos),
                                 engine._ptr(pose), engine._ptr(stat), engine._ptr(spread), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sgpr_last_error()
    raw.keep = (d_map, d_cols, d_T, d_acc, d_odo)          # (alive until the next call: the launch is asynchronous)
    return pose, stat, spread


def check(map_poses, cols, T, **kw):
    """the call against the reference -> the reference's (pose, stat, spread)"""
    got = raw(map_poses, cols, T, **kw)
    torch.cuda.synchronize()
    want = ref.localize(map_poses, cols, T, **kw)
    assert same(got[1], want[1]), "stat: rows %s differ" % np.flatnonzero((got[1].cpu().numpy() != want[1]).any(1))[:8]
    assert same(got[0], want[0]), "pose: %d of %d doubles differ" % (int((got[0].cpu().numpy() != want[0]).sum()), want[0].size)
    assert same(got[2], want[2]), "spread: rows %s differ" % np.flatnonzero(got[2].cpu().numpy() != want[2])[:8]
    return want


def world(seed, Q, K, **kw):
    from sg_pr_amd import synth
    return synth.localize_world(seed, map_scans=max(2 * Q, 40), queries=Q, k=K, **kw)


@pytest.fixture(scope="module")
def planted():
    from sg_pr_amd import synth
    return synth.localize_world(1)


# ------------------------------------------------------------------ 1. the planted world, slot counts, sessions
def test_planted_world_with_and_without_odometry(planted):
    from sg_pr_amd import localize, metrics
    w = planted
    pose, stat, _ = check(w["map"], w["cols"], w["T"], odo=w["odom"], L=8)
    acc = stat[:, 0] >= 5
    assert acc.mean() >= 0.97 and metrics.localization_errors(pose, w["truth"])["trans_m"][acc].max() <= 1.0
    want1 = check(w["map"], w["cols"], w["T"], odo=None, L=1)
    assert (want1[1][:, 0] >= 3).mean() <= 0.85
    # the Python surface: the same bits, the cosine formed from max_yaw, the dict and its accept
    got = localize.localize_async(w["map"], w["cols"], w["T"], odo=w["odom"], seq_len=8, max_trans=1.0, max_yaw=0.1)
    assert same(got[0], pose) and same(got[1], stat)
    d = localize.localize(w["map"], w["cols"], w["T"], seq_len=1, min_support=3)
    assert same(d["pose"], want1[0]) and same(d["support"], want1[1][:, 0]) and same(d["winner"], want1[1][:, 2])
    assert same(d["live"], want1[1][:, 1]) and same(d["flags"], want1[1][:, 3]) and same(d["spread"], want1[2])
    assert same(d["accept"], want1[1][:, 0] >= 3) and "accept" not in localize.localize(w["map"], w["cols"], w["T"])
    empty = localize.localize(w["map"], np.zeros((0, 8), np.int32), np.zeros((0, 8, 4)), min_support=1)
    assert tuple(empty["pose"].shape) == (0, 4) and tuple(empty["accept"].shape) == (0,)


@pytest.mark.parametrize("K,L,Q", [(1, 1, 9), (5, 3, 9), (8, 8, 12), (64, 1, 5), (33, 2, 5), (13, 5, 9), (64, 4, 7),
                                   (64, 16, 3), (64, 16, 17), (32, 16, 17), (16, 8, 10), (3, 16, 20)])
def test_slot_counts_at_every_block_size_boundary(K, L, Q):
    w = world(K * 100 + L, Q, K)
    stat = check(w["map"], w["cols"], w["T"], odo=w["odom"] if L > 1 else None, L=L)[1]
    assert stat[:, 1].max() >= min(L, Q) * K // 2 and (stat[:, 0] >= 1).all()
    if Q > L:
        assert stat[-1, 2] >= 0 and stat[:, 1].max() > (L - 1) * K        # a full window was seen


def test_session_tables():
    w = world(3, 12, 4, true_frac=0.7)
    one = check(w["map"], w["cols"], w["T"], odo=w["odom"], L=4)[1]
    two = check(w["map"], w["cols"], w["T"], odo=w["odom"], L=4, starts=[0, 1])[1]
    assert two[0, 1] <= 4 and two[1, 1] <= 4 and one[1, 1] >= two[1, 1] and (two[4:] == one[4:]).all()
    # 64 sessions over 80 queries: empty ones, one-query ones and a few longer
    lens = [(0, 1, 0, 3, 1, 0, 0, 5)[j % 8] for j in range(64)]
    starts = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int32)
    Q = int(np.sum(lens))
    w = world(4, Q, 5, true_frac=0.7)
    stat = check(w["map"], w["cols"], w["T"], odo=w["odom"], L=3, starts=starts)[1]
    lo = ref.session_lo(Q, starts)
    assert (stat[:, 1] <= 5 * np.minimum(3, np.arange(Q) - lo + 1)).all() and (stat[lo == np.arange(Q), 2] < 5).all()
    check(w["map"], w["cols"], w["T"], odo=w["odom"], L=3, starts=[0, Q, Q])          # sessions that start at the end


# ------------------------------------------------------------------ 2. maps, padding, masks
def test_empty_and_one_scan_maps():
    w = world(5, 6, 4)
    stat = check(np.zeros((0, 4)), w["cols"], w["T"], odo=w["odom"], L=2)[1]
    assert stat.tolist() == [[0, 0, -1, ref.NO_HYPOTHESIS]] * 6
    T = ref.compose(ref.inverse(w["map"][:1])[None], ref.compose(w["truth"][:, None, :], np.tile(IDENT, (6, 4, 1))))
    T[..., 2] += np.random.default_rng(0).normal(0, 0.1, (6, 4))
    stat = check(w["map"][:1], np.zeros((6, 4), np.int32), T, odo=w["odom"], L=2)[1]
    assert stat[:, 1].tolist() == [4, 8, 8, 8, 8, 8] and stat[1:, 0].min() >= 6


def test_padding_and_accept_masks():
    w = world(6, 10, 6, true_frac=0.8)
    M = w["map"].shape[0]
    cols = w["cols"].copy()
    cols[0, :] = -1
    cols[1, ::2] = M
    cols[2, 1:] = 0x7fffffff
    cols[3, 3] = -0x80000000
    cols[5] = [-1, M, 0x7fffffff, -7, M + 1, -1]
    kw = dict(odo=w["odom"], L=1)
    stat = check(w["map"], cols, w["T"], **kw)[1]
    assert stat[0].tolist() == [0, 0, -1, 1] == stat[5].tolist() and stat[1, 1] == 3 and stat[2, 1] == 1 and stat[3, 1] == 5
    stat = check(w["map"], cols, w["T"], odo=w["odom"], L=3)[1]
    assert stat[5, 1] == 11 and stat[0, 1] == 0 and stat[2, 1] == 4        # a query without candidates borrows its past
    none, every = np.zeros((10, 6), np.uint8), np.full((10, 6), 200, np.uint8)
    assert check(w["map"], w["cols"], w["T"], accept=none, odo=w["odom"], L=3)[1].tolist() == [[0, 0, -1, 1]] * 10
    assert same(check(w["map"], w["cols"], w["T"], accept=every, odo=w["odom"], L=3)[1],
                ref.localize(w["map"], w["cols"], w["T"], odo=w["odom"], L=3)[1])
    scattered = (np.arange(60).reshape(10, 6) * 7 % 5 < 2).astype(np.uint8)
    scattered[4] = 0
    stat = check(w["map"], w["cols"], w["T"], accept=scattered, odo=w["odom"], L=2)[1]
    assert (stat[:, 1] == scattered.sum(1) + np.concatenate(([0], scattered.sum(1)[:-1]))).all()


def test_nonfinite_inputs_kill_only_the_slots_they_touch():
    w = world(7, 8, 4, true_frac=1.0)
    kw = dict(odo=w["odom"], L=3)
    base = check(w["map"], w["cols"], w["T"], **kw)[1]
    assert base[:, 1].tolist() == [4, 8, 12, 12, 12, 12, 12, 12]
    for bad in (np.nan, np.inf, -np.inf):
        m = w["map"].copy()
        col = int(w["cols"][4, 1])
        m[col, 2] = bad
        uses = (w["cols"] == col).sum(1)
        stat = check(m, w["cols"], w["T"], **kw)[1]
        assert (base[:, 1] - stat[:, 1] == uses + np.concatenate(([0], uses[:-1])) + np.concatenate(([0, 0], uses[:-2]))).all()
        T = w["T"].copy()
        T[3, 2, 1] = bad
        stat = check(w["map"], w["cols"], T, **kw)[1]
        assert (base[:, 1] - stat[:, 1]).tolist() == [0, 0, 0, 1, 1, 1, 0, 0]
        odo = w["odom"].copy()
        odo[4, 3] = bad
        # as odo[i]: query 4 keeps l = 0 alone; as odo[j]: queries 5 and 6 lose the slots carried over from scan 4
        stat = check(w["map"], w["cols"], w["T"], odo=odo, L=3)[1]
        assert stat[:, 1].tolist() == [4, 8, 12, 12, 4, 8, 8, 12]
        want1 = ref.localize(w["map"], w["cols"], w["T"], L=1)
        got = raw(w["map"], w["cols"], w["T"], odo=odo, L=3, starts=[0, 4])
        assert same(got[0][4], want1[0][4]) and same(got[1][4], want1[1][4])


# ------------------------------------------------------------------ 3. decisions exactly at a tolerance
def two_places(a, b, **kw):
    return check(np.array([a, b], np.float64), np.array([[0, 1]]), np.tile(IDENT, (1, 2, 1)), **kw)


def test_translation_exactly_at_the_tolerance():
    a, b = [1.0, 0.0, 10.0, -2.0], [1.0, 0.0, 13.0, 2.0]
    assert two_places(a, b, max_trans=5.0)[1].tolist() == [[2, 2, 0, 0]]
    assert two_places(a, b, max_trans=np.nextafter(5.0, 0.0))[1].tolist() == [[1, 2, 0, 0]]
    assert two_places(b, a, max_trans=5.0)[1].tolist() == [[2, 2, 0, 0]]
    assert two_places(a, a, max_trans=0.0)[1].tolist() == [[2, 2, 0, 0]]
    assert two_places(a, b, max_trans=np.inf)[1].tolist() == [[2, 2, 0, 0]]


def test_rotation_exactly_at_the_tolerance():
    c = math.cos(0.1)
    a, b = [1.0, 0.0, 0.0, 0.0], [c, math.sin(0.1), 0.0, 0.0]           # the dot product is c, exactly
    assert two_places(a, b, min_cos=c)[1].tolist() == [[2, 2, 0, 0]]
    assert two_places(a, b, min_cos=np.nextafter(c, -2.0))[1].tolist() == [[2, 2, 0, 0]]       # the dot one ulp above
    assert two_places(a, b, min_cos=np.nextafter(c, 2.0))[1].tolist() == [[1, 2, 0, 0]]        # ... and one ulp below
    assert two_places(b, a, min_cos=c)[1].tolist() == [[2, 2, 0, 0]]
    assert two_places(a, b, min_cos=-np.inf)[1].tolist() == [[2, 2, 0, 0]]
    assert two_places(a, b, min_cos=np.inf)[1].tolist() == [[1, 2, 0, 0]]


def test_duplicated_hypotheses_and_equal_supports():
    w = world(8, 6, 8, true_frac=0.5)
    cols, T = np.repeat(w["cols"], 4, axis=1), np.repeat(w["T"], 4, axis=1)            # every candidate four times
    stat = check(w["map"], cols, T, odo=w["odom"], L=2)[1]
    assert (stat[:, 0] % 4 == 0).all() and (stat[:, 2] % 4 == 0).all()
    # two clusters of two: the lowest slot wins; three against two: the three
    m = np.array([[1, 0, 5, 5], [1, 0, 0, 0], [1, 0, 0, 0.1], [1, 0, 5, 5.1], [1, 0, 0.1, 0.1]], np.float64)
    assert check(m, np.array([[0, 1, 2, 3]]), np.tile(IDENT, (1, 4, 1)))[1].tolist() == [[2, 4, 0, 0]]
    assert check(m, np.array([[0, 1, 2, 3, 4]]), np.tile(IDENT, (1, 5, 1)))[1].tolist() == [[3, 5, 1, 0]]


def test_opposite_headings_are_degenerate():
    m = np.array([[1.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 0.5, 0.0]])
    pose, stat, spread = check(m, np.array([[1, 0]]), np.tile(IDENT, (1, 2, 1)), min_cos=-1.0)
    assert stat.tolist() == [[2, 2, 0, ref.DEGENERATE]] and pose[0].tolist() == [-1.0, 0.0, 0.25, 0.0] and spread[0] == 0.25
    # sums that overflow are reported as they come
    big = np.array([[1.0, 0.0, 1.7e308, 0.0], [1.0, 0.0, 1.7e308, 0.0]])
    check(big, np.array([[0, 1]]), np.tile(IDENT, (1, 2, 1)), max_trans=np.inf)


# ------------------------------------------------------------------ 4. streams
def test_two_streams_give_the_same_bits(planted):
    w = planted
    want = ref.localize(w["map"], w["cols"], w["T"], odo=w["odom"], L=8)
    got, kept = [], []
    for _ in range(2):
        got.append(raw(w["map"], w["cols"], w["T"], odo=w["odom"], L=8, stream=torch.cuda.Stream()))
        kept.append(raw.keep)
    torch.cuda.synchronize()
    for pose, stat, spread in got:
        assert same(pose, want[0]) and same(stat, want[1]) and same(spread, want[2])


# ------------------------------------------------------------------ 5. the model's surface and the command line
@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_sg_localize_end_to_end(model):
    """a 240-scan world: the first two thirds with their true poses are the map, the last third re-drives the first and
    is the query drive, its odometry in a frame of its own: retrieved, verified, localised.  Equality with the reference
    run on the verified records; the accepted queries land on the truth."""
    from sg_pr_amd import metrics, synth
    centers, labels, _, poses = synth.world_sequence(240, 100, seed=6)
    a, b = slice(0, 160), slice(160, 240)
    pooled = model.embed(centers, labels)[0]
    vals, idx = model.loop_closures(pooled[b], pooled[a], k=4)
    ver = model.verify_closures(centers[b], labels[b], idx, values=vals, min_inliers=12, col_centers=centers[a],
                                col_labels=labels[a])
    Xa, Xb = metrics.planar_odometry(poses[a]), metrics.planar_odometry(poses[b])
    own = synth._se2_compose(np.array([[math.cos(2.3), math.sin(2.3), -310.0, 95.0]]), Xb)
    host = {k: ver[k].cpu().numpy() for k in ("refined", "flags", "accept")}
    for L, S, query_poses in ((4, 3, own), (1, 2, None)):
        loc = model.localize(ver, idx, poses[a], query_poses=query_poses, seq_len=L, min_support=S)
        want = ref.localize_verified(host["refined"], host["flags"], host["accept"], idx.cpu().numpy(), Xa, odo=query_poses,
                                     L=L, min_support=S)
        for key in ("pose", "support", "live", "winner", "flags", "spread", "accept"):
            assert same(loc[key], want[key]), (L, key)
        acc = want["accept"]
        err = metrics.localization_errors(want["pose"], Xb)
        print("L = %d, support >= %d: accepted %d of 80, translation error median %.3f m, largest %.3f m"
              % (L, S, acc.sum(), np.median(err["trans_m"][acc]), err["trans_m"][acc].max()))
        assert acc.sum() >= 1 and np.median(err["trans_m"][acc]) < 1.0
    with pytest.raises(ValueError, match="odometry"):
        model.localize(ver, idx, poses[a], seq_len=2)


def test_place_db_localize_cli(model, tmp_path, ckpt_path, capsys):
    """--verify --localize: the file holds the reference's answer for the records written beside it"""
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
    place_db.main([str(cfg), "--k", "3", "--window", "30", "--verify", "--min-inliers", "15", "--localize", "--loc-len", "4",
                   "--min-support", "3", "--loc-max-trans", "0.8", "--loc-max-yaw-deg", "4"])
    line = next(l for l in capsys.readouterr().out.splitlines() if "localised" in l)
    z = np.load(tmp_path / "eva" / "07_localize.npz")
    X = metrics.planar_odometry(poses)
    assert int(z["seq_len"]) == 4 and int(z["min_support"]) == 3 and z["indices"].shape == (150, 3)
    want = ref.localize_verified(z["refined"], z["verify_flags"], z["verify_accept"], z["indices"], X, odo=X, L=4,
                                 max_trans=float(z["max_trans"]), max_yaw=float(z["max_yaw"]), min_support=3)
    assert float(z["max_trans"]) == 0.8 and float(z["max_yaw"]) == math.radians(4.0)
    for key in ("pose", "support", "live", "winner", "flags", "spread", "accept"):
        assert same(z[key], want[key]), key
    acc = want["accept"]
    assert acc.sum() >= 1 and "localised %.4f of 150 scans (last 4 scans, support >= 3)" % acc.mean() in line
    err = metrics.localization_errors(want["pose"], X)["trans_m"][acc]
    assert "translation error median %.3f m, 95%% %.3f m" % (np.median(err), np.percentile(err, 95)) in line
    assert "best verified candidate alone: %.4f" % z["single_accept"].mean() in line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--localize"])
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--verify", "--localize", "--loc-len", "17"])
