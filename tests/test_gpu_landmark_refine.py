"""The landmark refinement on the GPU (sgpr_landmark_refine, include/sgpr_landmark_refine.h): poses, costs
and info equal to the NumPy definition (tests/landmark_refine_ref.py) to the bit - at the shapes where the launch and a
lane's slot count change, at iteration counts that use both accumulator sets and their clearing, on the planted world,
on the boundaries of the keep rule, with unused nodes of every kind and heavy contention on one landmark - then
order-freedom, streams, the Python layer, the pipeline end to end and the command line.  Every output and the workspace
are pre-filled with 0xFF, and the outputs carry a margin that must stay 0xFF."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_ref as lref  # noqa: E402
import landmark_refine_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
MARGIN = 5


def device_refine(centers, node_landmark, poses, lm_use, fixed=None, iters=10, min_nodes=6, stream=None, ws_fill=0xFF,
                  out_fill=0xFF, workspace=None):
    """the C call with every output (and a margin behind it) full of the byte out_fill and the workspace full of ws_fill
    (a given workspace is used as it is) -> dict of host arrays"""
    from sg_pr_amd import engine, landmarks
    lib = landmarks.load_library()
    dev = torch.device("cuda", 0)
    node = torch.as_tensor(np.ascontiguousarray(node_landmark, np.int32)).to(dev)
    G, N = node.shape
    cen = torch.as_tensor(np.ascontiguousarray(centers, F32).reshape(G, N, 3)).to(dev)
    X = torch.as_tensor(np.ascontiguousarray(poses, np.float64).reshape(G, 4)).to(dev)
    use = torch.as_tensor(np.ascontiguousarray(lm_use, np.uint8).reshape(-1)).to(dev)
    L = use.numel()
    fix = None if fixed is None else torch.as_tensor(np.ascontiguousarray(fixed, np.uint8).reshape(G)).to(dev)

    def dirty(n, dtype):
        return torch.full((n * dtype.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(dtype)

    out = {"poses": dirty(4 * (G + MARGIN), torch.float64), "cost": dirty(iters + 1 + MARGIN, torch.float64),
           "info": dirty(4 + MARGIN, torch.int32)}
    need = landmarks.refine_workspace_bytes(G, N, L)
    assert need == ref.workspace_bytes(G, N, L)
    ws = torch.full((max(need, 1),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs and the fills were made on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_landmark_refine(p(cen), G, N, p(X), p(node), p(use) if L else None, L, p(fix), int(iters), int(min_nodes),
                                      p(out["poses"]), p(out["cost"]), p(out["info"]), p(ws), need, engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(centers, node_landmark, poses, lm_use, **kw):
    """the device call equals the reference to the bit (NaN as NaN: bytes), nothing written past the outputs"""
    kw.pop("stream", None)
    extra = {k: kw.pop(k) for k in ("ws_fill", "out_fill", "workspace") if k in kw}
    out_fill = extra.get("out_fill", 0xFF)
    got = device_refine(centers, node_landmark, poses, lm_use, **extra, **kw)
    want = ref.refine(centers, node_landmark, poses, lm_use, **kw)
    G, N = np.asarray(node_landmark).shape
    T = want["cost"].size - 1
    if G * N == 0:
        assert all((v.view(np.uint8) == out_fill).all() for v in got.values())        # nothing is written
        return want
    assert got["cost"][:T + 1].tobytes() == want["cost"].tobytes(), (got["cost"][:T + 1], want["cost"])
    assert got["info"][:4].tolist() == want["info"].tolist()
    assert got["poses"][:4 * G].tobytes() == want["poses"].tobytes()
    for name, n in (("poses", 4 * G), ("cost", T + 1), ("info", 4)):
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"
    return want


def make_case(G, N, seed, noise=0.1, perturb=0.2):
    """G scans of N nodes that observe G N / 4 planted points from perturbed poses; a few ids are -1 or past L, one
    landmark in ten is not in use -> (centers, node_landmark, poses, lm_use)"""
    rng = np.random.default_rng(seed)
    L = max(1, (G * N) // 4)
    pts = rng.uniform(-20.0, 20.0, size=(L, 2))
    ids = rng.integers(0, L, size=(G, N))
    yaw = rng.uniform(-3.0, 3.0, size=G)
    t = rng.uniform(-5.0, 5.0, size=(G, 2))
    d = pts[ids] + rng.normal(0.0, noise, size=(G, N, 2)) - t[:, None, :]
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    centers = np.stack((c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0], rng.uniform(-1, 1, size=(G, N))), axis=-1)
    yaw = yaw + rng.normal(0.0, 0.1 * perturb, size=G)
    t = t + rng.normal(0.0, perturb, size=(G, 2))
    poses = np.stack((np.cos(yaw), np.sin(yaw), t[:, 0], t[:, 1]), axis=1)
    ids = np.where(rng.random((G, N)) < 0.05, -1, ids)
    ids = np.where(rng.random((G, N)) < 0.05, L + rng.integers(0, 3, size=(G, N)), ids)
    use = (rng.random(L) < 0.9).astype(np.uint8)
    return centers.astype(F32), ids.astype(np.int32), poses, use


@pytest.fixture(scope="module")
def worlds():
    from sg_pr_amd import synth
    return {seed: synth.landmark_world(seed) for seed in (0, 1)}


# ------------------------------------------------------------------ shapes and iteration counts
@pytest.mark.parametrize("G,N", [(1, 1), (1, 3), (2, 64), (3, 65), (5, 130), (17, 100)])
def test_shapes(G, N):
    case = make_case(G, N, G * 1000 + N)
    fixed = np.zeros(G, np.uint8)
    fixed[0] = 1
    for T in (0, 1, 2, 7):
        want = check(*case, iters=T, min_nodes=2, fixed=fixed if G > 1 else None)
        if G * N >= 128 and T >= 1:
            assert want["info"][2] >= G - 1 and want["cost"][T] < want["cost"][0]


def test_no_slots():
    check(np.zeros((4, 0, 3), F32), np.zeros((4, 0), np.int32), np.tile((1.0, 0, 0, 0), (4, 1)), np.ones(3, np.uint8), iters=2)


@pytest.mark.parametrize("seed", [0, 1])
def test_world(worlds, seed):
    from sg_pr_amd import synth
    w = worlds[seed]
    rng = np.random.default_rng(50 + seed)
    G = w["truth"].shape[0]
    start = synth._se2_compose(w["truth"], synth._se2(rng.normal(0, 0.004, G), rng.normal(0, 0.03, G), rng.normal(0, 0.03, G)))
    lm = lref.landmark_map(w["centers"], w["labels"], start, starts=w["starts"])
    fixed = np.zeros(G, np.uint8)
    fixed[0] = 1
    want = check(w["centers"], lm["node_landmark"], start, (lm["count"] >= 2).astype(np.uint8), fixed=fixed, iters=10)
    assert want["info"][0] > 10000 and want["info"][2] == G - 1 and want["cost"][-1] < want["cost"][0]
    assert want["poses"][0].tobytes() == start[0].tobytes()


# ------------------------------------------------------------------ the keep rule
def test_min_nodes_at_the_count():
    centers, ids, poses, use = make_case(4, 20, 7)
    use[:] = 1
    ids[2, 9:] = -1                                              # scan 2 has exactly 9 used nodes
    ids[2, :9] = np.clip(ids[2, :9], 0, use.size - 1)
    for mn, moved in ((8, True), (9, True), (10, False)):
        want = check(centers, ids, poses, use, iters=2, min_nodes=mn)
        assert (want["poses"][2].tobytes() != poses[2].tobytes()) == moved, mn


def test_fixed_scans():
    case = make_case(6, 40, 21)
    poses = case[2]
    want = check(*case, iters=3, fixed=np.ones(6, np.uint8))
    assert want["poses"].tobytes() == poses.tobytes() and want["info"][2:].tolist() == [0, 0]
    assert want["cost"][3] == want["cost"][0]
    none = check(*case, iters=3, fixed=np.zeros(6, np.uint8))
    null = check(*case, iters=3, fixed=None)
    assert none["poses"].tobytes() == null["poses"].tobytes() and none["info"][2] == 6
    some = check(*case, iters=3, fixed=np.array([0, 1, 0, 0, 1, 0], np.uint8))
    assert some["poses"][[1, 4]].tobytes() == poses[[1, 4]].tobytes() and some["info"][2:].tolist() == [4, 0]


def test_ids_outside_the_landmarks_and_masks():
    centers, ids, poses, use = make_case(5, 33, 3)
    ids[0, :] = -1                                               # a scan without a single used node keeps its pose
    ids[1, ::2] = use.size
    ids[1, 1::4] = 0x7fffffff
    ids[2, 0] = -0x80000000
    want = check(centers, ids, poses, use, iters=2, min_nodes=2)
    assert want["poses"][0].tobytes() == poses[0].tobytes() and want["info"][3] >= 1
    off = check(centers, ids, poses, np.zeros_like(use), iters=2, min_nodes=2)
    assert np.isnan(off["cost"]).all() and off["poses"].tobytes() == poses.tobytes() and off["info"].tolist() == [0, 0, 0, 5]
    none = check(centers, ids, poses, np.zeros(0, np.uint8), iters=1, min_nodes=2)           # L == 0, a NULL mask
    assert np.isnan(none["cost"]).all() and none["info"].tolist() == [0, 0, 0, 5]


def test_contention_on_one_landmark():
    centers, ids, poses, use = make_case(6, 100, 8)
    ids[:, :50] = 0                                              # 300 observations of landmark 0, wherever they lie
    use[0] = 1
    want = check(centers, ids, poses, use, iters=3, min_nodes=2)
    assert want["info"][0] > 450 and want["info"][2] == 6
    # one landmark alone, 300 observations: three adjacent waves' worth of atomics on one address
    want = check(centers[:3], np.zeros((3, 100), np.int32), poses[:3], np.ones(1, np.uint8), iters=2, min_nodes=2)
    assert want["info"][:2].tolist() == [300, 1]


def test_non_finite_poses_and_centres():
    centers, ids, poses, use = make_case(8, 24, 13)
    use[:] = 1
    poses[1, 0] = np.nan
    poses[2, 3] = np.inf
    poses[3, 1] = -np.inf
    centers[4, 3, 0] = np.nan
    centers[4, 5, 1] = np.inf
    centers[5, :, 0] = F32(3e38)                                 # finite, and past the limit once in the map frame
    poses[6] = (1.0, 0.0, 2.0 ** 37, 0.0)
    want = check(centers, ids, poses, use, iters=3, min_nodes=2)
    assert want["poses"][[1, 2, 3, 5]].tobytes() == poses[[1, 2, 3, 5]].tobytes()
    assert np.isfinite(want["cost"]).all() and np.isfinite(want["poses"][[0, 4, 7]]).all()
    assert want["poses"][4].tobytes() != poses[4].tobytes()


# ------------------------------------------------------------------ order, streams
def test_scan_order_decides_nothing():
    centers, ids, poses, use = make_case(17, 100, 5)
    fixed = np.zeros(17, np.uint8)
    fixed[3] = 1
    perm = np.random.default_rng(9).permutation(17)
    a = device_refine(centers, ids, poses, use, fixed=fixed, iters=4)
    b = device_refine(centers[perm], ids[perm], poses[perm], use, fixed=fixed[perm], iters=4)
    assert a["poses"][:68].reshape(17, 4)[perm].tobytes() == b["poses"][:68].tobytes()
    assert a["cost"].tobytes() == b["cost"].tobytes() and a["info"].tobytes() == b["info"].tobytes()


def test_two_streams_two_dirty_workspaces():
    case = make_case(17, 100, 6)
    outs = [device_refine(*case, iters=5, stream=torch.cuda.Stream()) for _ in range(2)]
    want = ref.refine(*case, iters=5)
    for o in outs:
        assert o["poses"][:68].tobytes() == want["poses"].tobytes() and o["cost"][:6].tobytes() == want["cost"].tobytes()


# ------------------------------------------------------------------ the Python layer
def test_python_layer_and_a_short_workspace(worlds):
    from sg_pr_amd import landmarks
    w = worlds[0]
    lm = landmarks.build(w["centers"], w["labels"], w["odom"], starts=w["starts"])
    use = landmarks.select(lm, min_count=2)
    fixed = np.zeros(300, bool)
    fixed[0] = True
    X, info = landmarks.refine(w["centers"], w["labels"], w["odom"], lm, use=use, fixed=fixed, iters=3)
    want = ref.refine(w["centers"], lm["node_landmark"].cpu().numpy(), w["odom"], use.cpu().numpy(), fixed=fixed, iters=3)
    assert X.is_cuda and X.cpu().numpy().tobytes() == want["poses"].tobytes()
    assert info["cost"].tobytes() == want["cost"].tobytes()
    assert [info[k] for k in ("used_nodes", "landmarks", "refitted", "kept")] == want["info"].tolist()
    every = landmarks.refine_async(w["centers"], w["labels"], w["odom"], lm, iters=1)
    want = ref.refine(w["centers"], lm["node_landmark"].cpu().numpy(), w["odom"], np.ones(lm["num_landmarks"], np.uint8), iters=1)
    assert every["poses"].cpu().numpy().tobytes() == want["poses"].tobytes()
    short = torch.empty(landmarks.refine_workspace_bytes(300, 100, lm["num_landmarks"]) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception, match="workspace"):
        landmarks.refine_async(w["centers"], w["labels"], w["odom"], lm, workspace=short)


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_pipeline_end_to_end(model, worlds):
    """verify the world's true closures, select, optimise, refine: the refined map is sharper than the geometric mean of
    the optimised and the true-pose sharpness of this run - halfway between what the stage must separate (DESIGN.md §27
    recorded 0.293 and 0.214 m) - and the trajectory is nearer the truth than the optimised one"""
    from sg_pr_amd import metrics
    w = worlds[0]
    rows, cols = w["rows"].astype(np.int64), w["cols"].astype(np.int64)
    ver = model.verify_closures(w["centers"][rows], w["labels"][rows], cols[:, None], min_inliers=12,
                                col_centers=w["centers"], col_labels=w["labels"])
    sel = model.consistent_closures(ver, rows[:, None], cols[:, None], w["odom"], row_sessions=w["starts"],
                                    col_sessions=w["starts"])
    X, _ = model.optimize_map(sel, ver, rows[:, None], cols[:, None], w["odom"], sessions=w["starts"])
    Y, lm, costs = model.refine_map(w["centers"], w["labels"], X, sessions=w["starts"])
    opt = metrics.map_sharpness(model.landmark_map(w["centers"], w["labels"], X, sessions=w["starts"]))["sharpness"]
    tru = metrics.map_sharpness(lref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"]))["sharpness"]
    got = metrics.map_sharpness(lm)["sharpness"]
    e_opt, e_ref = metrics.trajectory_error(X, w["truth"]), metrics.trajectory_error(Y, w["truth"])
    print("sharpness: optimised %.4f, refined %.4f, true poses %.4f (bound %.4f); trajectory error %.4f -> %.4f m; cost %s"
          % (opt, got, tru, math.sqrt(opt * tru), e_opt, e_ref, [np.round(c, 4).tolist() for c in costs]))
    assert len(costs) == 2 and all(c.shape == (11,) for c in costs)
    assert Y[0].cpu().numpy().tobytes() == X[0].cpu().numpy().tobytes()
    # the two rounds are the reference's, to the bit
    Z = X.cpu().numpy()
    for r in range(2):
        m = lref.landmark_map(w["centers"], w["labels"], Z, starts=w["starts"])
        fixed = np.zeros(300, bool)
        fixed[0] = True
        out = ref.refine(w["centers"], m["node_landmark"], Z, (m["count"] >= 2).astype(np.uint8), fixed=fixed, iters=10)
        assert out["cost"].tobytes() == costs[r].tobytes()
        Z = out["poses"]
    assert Z.tobytes() == Y.cpu().numpy().tobytes()
    assert got < math.sqrt(opt * tru)
    assert e_ref < e_opt


def test_place_db_refine_cli(model, tmp_path, ckpt_path, capsys):
    """--landmarks --refine: the poses file holds the reference's refinement of the sequence's own poses, the landmark
    file the reference's map on them, the line the figures of both"""
    from sg_pr_amd import graph_store, metrics, place_db, synth
    centers, labels, _, poses = synth.world_sequence(90, 100, seed=4)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(90)])
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
    saved = tmp_path / "refined.npy"
    place_db.main([str(cfg), "--window", "30", "--landmarks", "--refine", "--refine-rounds", "2", "--refine-iters", "4",
                   "--save-poses", str(saved)])
    lines = capsys.readouterr().out.splitlines()
    own = metrics.planar_odometry(poses)
    Z = own
    fixed = np.zeros(90, bool)
    fixed[0] = True
    for _ in range(2):
        m = lref.landmark_map(centers, labels, Z)
        Z = ref.refine(centers, m["node_landmark"], Z, (m["count"] >= 2).astype(np.uint8), fixed=fixed, iters=4)["poses"]
    assert np.load(saved).tobytes() == Z.tobytes() and (Z[1:] != own[1:]).any()
    z = np.load(tmp_path / "eva" / "07_landmarks.npz")
    want = lref.landmark_map(centers, labels, Z)
    for name in ("center", "label", "count", "first", "spread", "node_landmark"):
        assert z[name].tobytes() == want[name].tobytes(), name
    assert z["poses"].tobytes() == Z.tobytes()
    before, after = metrics.map_sharpness(lref.landmark_map(centers, labels, own)), metrics.map_sharpness(want)
    line = next(l for l in lines if "refined on its landmarks" in l)
    assert "2 x 4 iterations" in line
    assert "landmarks %d -> %d, sharpness %.4f m -> %.4f m, shared %.4f -> %.4f" % (
        before["landmarks"], after["landmarks"], before["sharpness"], after["sharpness"], before["shared"], after["shared"]) in line
    assert "trajectory error %.4f m -> %.4f m" % (0.0, metrics.trajectory_error(Z, own)) in line
    line = next(l for l in lines if "landmark map of" in l)
    assert "landmarks %d sharpness %.4f m" % (after["landmarks"], after["sharpness"]) in line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--refine"])
