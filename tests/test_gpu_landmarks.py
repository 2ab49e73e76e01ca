"""The landmark map on the GPU (sgpr_landmark_map, include/sgpr_landmarks.h): every output equal to the
NumPy definition (tests/landmark_ref.py) to the bit - on the planted world, at the shapes where the launch changes, on
the boundaries of every rule, on deep forests and heavy cells, with dead nodes of every kind, at every capacity, with 64
sessions - then order-freedom, streams, the Python layer and the pipeline end to end.  Every output and the workspace
are pre-filled with 0xFF."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

IDENT = (1.0, 0.0, 0.0, 0.0)
F32 = np.float32


def device_map(centers, labels, poses, starts=None, radius=0.75, tau_z=0.75, n_labels=12, max_landmarks=None, stream=None,
               ws_fill=0xFF, out_fill=0xFF, workspace=None):
    """the C call with every output full of the byte out_fill and the workspace full of ws_fill (a given workspace is used
    as it is) -> dict of host arrays (all max_landmarks rows)"""
    from sg_pr_amd import engine, landmarks
    lib = landmarks.load_library()
    dev = torch.device("cuda", 0)
    lab = torch.as_tensor(np.ascontiguousarray(labels, np.int32)).to(dev)
    G, N = lab.shape
    cen = torch.as_tensor(np.ascontiguousarray(centers, F32).reshape(G, N, 3)).to(dev)
    X = torch.as_tensor(np.ascontiguousarray(poses, np.float64).reshape(G, 4)).to(dev)
    rad = np.atleast_1d(np.asarray(radius, np.float64))
    rad = np.ascontiguousarray(np.full(n_labels, rad[0]) if rad.size == 1 else rad)
    cap = G * N if max_landmarks is None else int(max_landmarks)
    table = None if starts is None else np.ascontiguousarray(starts, np.int32)

    def dirty(shape, dtype):
        return torch.full((math.prod(shape) * dtype.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)

    out = {"center": dirty((cap, 3), torch.float64), "label": dirty((cap,), torch.int32), "count": dirty((cap,), torch.int32),
           "first": dirty((cap,), torch.int32), "sessions": dirty((cap,), torch.int64), "spread": dirty((cap,), torch.float64),
           "node_landmark": dirty((G, N), torch.int32), "num": dirty((2,), torch.int32)}
    need = landmarks.workspace_bytes(G, N)
    assert need == ref.workspace_bytes(G, N)
    ws = torch.full((max(need, 1),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs and the fills were made on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_landmark_map(p(cen), p(lab), G, N, p(X), None if table is None else table.ctypes.data,
                                   0 if table is None else table.shape[0], rad.ctypes.data, rad.shape[0], float(tau_z), cap,
                                   p(out["center"]), p(out["label"]), p(out["count"]), p(out["first"]), p(out["sessions"]),
                                   p(out["spread"]), p(out["node_landmark"]), p(out["num"]), p(ws), need,
                                   engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(centers, labels, poses, **kw):
    """the device call equals the reference: records to the bit (NaN as NaN: bytes), nothing written past them"""
    extra = {k: kw.pop(k) for k in ("stream", "ws_fill", "out_fill", "workspace") if k in kw}
    out_fill = extra.get("out_fill", 0xFF)
    got = device_map(centers, labels, poses, **extra, **kw)
    want = ref.landmark_map(centers, labels, poses, **kw)
    labels = np.asarray(labels)
    if labels.size:
        assert got["num"].tolist() == want["num"].tolist()
        assert got["node_landmark"].tobytes() == want["node_landmark"].tobytes()
    else:
        assert (got["num"].view(np.uint8) == out_fill).all()      # nothing is written
    k = want["label"].shape[0]
    for name in ("center", "label", "count", "first", "sessions", "spread"):
        g = got[name]
        assert g[:k].tobytes() == want[name].tobytes(), name
        assert (g[k:].view(np.uint8) == out_fill).all(), name + ": written past the records"
    return want


def flat_scene(points, labels, shape=None):
    """points [(x, y, z)] and their labels as one scan per point (or `shape` = (G, N)) under identity poses"""
    pts = np.asarray(points, F32).reshape(-1, 3)
    G, N = shape or (pts.shape[0], 1)
    return pts.reshape(G, N, 3), np.asarray(labels, np.int32).reshape(G, N), np.tile(IDENT, (G, 1))


@pytest.fixture(scope="module")
def worlds():
    from sg_pr_amd import synth
    return {seed: synth.landmark_world(seed) for seed in (0, 1)}


# ------------------------------------------------------------------ the world
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("poses", ["truth", "odom"])
def test_world(worlds, seed, poses):
    w = worlds[seed]
    want = check(w["centers"], w["labels"], w[poses], starts=w["starts"])
    assert want["num"][1] > 10000 and want["links"] > 1000


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("G,N", [(1, 1), (1, 2), (2, 1), (3, 64), (65, 5), (17, 100)])
def test_shapes(G, N):
    rng = np.random.default_rng(G * 1000 + N)
    centers = rng.uniform(-6.0, 6.0, size=(G, N, 3)).astype(F32)
    centers[..., 2] = rng.uniform(-1.0, 1.0, size=(G, N))
    labels = rng.integers(-1, 4, size=(G, N)).astype(np.int32)
    yaw = rng.uniform(-3.0, 3.0, size=G)
    poses = np.stack((np.cos(yaw), np.sin(yaw), rng.uniform(-3, 3, size=G), rng.uniform(-3, 3, size=G)), axis=1)
    want = check(centers, labels, poses, radius=1.0)
    if G * N >= 192:
        assert 1 < want["num"][0] < want["num"][1]                # something fused, something not


def test_no_slots():
    check(np.zeros((4, 0, 3), F32), np.zeros((4, 0), np.int32), np.tile(IDENT, (4, 1)))


# ------------------------------------------------------------------ boundaries
def test_radius_boundary():
    scene = flat_scene([(0, 0, 0), (3, 4, 0)], [2, 2])
    assert check(*scene, radius=5.0)["num"].tolist() == [1, 2]
    assert check(*scene, radius=np.nextafter(5.0, 0.0))["num"].tolist() == [2, 2]


def test_height_boundary():
    assert check(*flat_scene([(0, 0, 0), (0.1, 0, 0.75)], [0, 0]), tau_z=0.75)["num"].tolist() == [1, 2]
    above = float(np.nextafter(F32(0.75), F32(1.0)))
    assert check(*flat_scene([(0, 0, 0), (0.1, 0, above)], [0, 0]), tau_z=0.75)["num"].tolist() == [2, 2]
    assert check(*flat_scene([(0, 0, -above), (0.1, 0, 0)], [0, 0]), tau_z=0.75)["num"].tolist() == [2, 2]


def test_cell_borders():
    w = max(0.75 * 1.001, 0.5)                                   # the cell width of radius 0.75
    # nodes on both sides of a border, along x, along y and across a corner
    pts = [(3 * w - 0.01, 0, 0), (3 * w + 0.01, 0, 0), (10, -2 * w - 0.01, 0), (10, -2 * w + 0.01, 0),
           (20 + 5 * w - 0.2, 5 * w - 0.2, 0), (20 + 5 * w + 0.2, 5 * w + 0.2, 0)]
    assert check(*flat_scene(pts, [1] * 6))["num"].tolist() == [3, 6]
    # a coordinate exactly on a border: the centre is 0 and the pose carries k w in float64
    centers, labels = np.zeros((4, 1, 3), F32), np.ones((4, 1), np.int32)
    poses = np.array([(1, 0, 3 * w, 0), (1, 0, 3 * w - 0.1, 0), (1, 0, 50.0, -7 * w), (1, 0, 50.0, -7 * w + 0.1)])
    assert check(centers, labels, poses)["num"].tolist() == [2, 4]


def test_negative_coordinates_and_zeros():
    pts = [(-0.0, 0.0, 0), (0.0, -0.0, 0), (-0.3, -0.3, 0), (0.3, 0.3, 0), (-0.74, 0, -0.0), (-1.6, 0.0, 0),
           (-100.2, -50.1, 0), (-100.4, -50.3, 0)]
    want = check(*flat_scene(pts, [0] * 8))
    assert want["num"].tolist() == [3, 8] and want["count"].tolist() == [5, 1, 2]


# ------------------------------------------------------------------ chains and cells
def test_long_chain_in_shuffled_order():
    r = 0.75
    x = np.arange(1000) * (0.9 * r)
    order = np.random.default_rng(5).permutation(1000)
    pts = np.stack((x[order], np.zeros(1000), np.zeros(1000)), axis=1)
    want = check(*flat_scene(pts, [3] * 1000, shape=(250, 4)))
    assert want["num"].tolist() == [1, 1000] and want["count"].tolist() == [1000]


def test_heavy_cells():
    r = 0.75
    pile = np.tile([(4.0, -9.0, 0.5)], (300, 1))
    want = check(*flat_scene(pile, [7] * 300, shape=(3, 100)))
    assert want["num"].tolist() == [1, 300] and want["spread"].tolist() == [0.0]
    two = np.concatenate((pile, pile + [1.01 * r, 0.0, 0.0]))
    want = check(*flat_scene(two, [7] * 600, shape=(6, 100)))
    assert want["num"].tolist() == [2, 600] and want["count"].tolist() == [300, 300]


# ------------------------------------------------------------------ more than 1024 workgroups
def test_numbering_scan_with_segments_of_two_workgroups():
    """1025 workgroups of 256 nodes: every thread of the one-workgroup numbering scan owns a SEGMENT of two workgroup
    counts, which no smaller map reaches.  The expected values are closed forms, not the reference's (its pure-Python
    linking would take minutes here): the nodes lie on a lattice of pitch 2 > radius, so every live node is its own
    landmark - its centre is its point exactly, its spread 0 - but for two planted pairs 0.5 apart, one across the
    workgroups 0 | 1 (nodes 255, 256: inside thread 0's segment), one across the workgroups 601 | 602 (nodes 154111,
    154112: the last of thread 300's segment and the first of thread 301's).  263 nodes are dead at the indices
    100 + 1000 k, so an id is "live roots before me", never the index."""
    G, N, ROW = 1025, 256, 512
    P = G * N
    p = np.arange(P)
    pts = np.stack((2.0 * (p % ROW), 2.0 * (p // ROW), 0.125 * (p % 7)), axis=1)
    labels = (p % 3).astype(np.int32)
    pairs = [(255, 256), (602 * N - 1, 602 * N)]
    for a, b in pairs:
        pts[b] = pts[a] + (0.5, 0.0, 0.0)
        labels[b] = labels[a]
    dead = np.arange(100, P, 1000)
    labels[dead[0::2]] = -1
    labels[dead[1::2]] = 12                                       # n_labels = 12: out of range
    assert dead.size == 263 and not set(dead) & {i + d for pr in pairs for i in pr for d in (-1, 0, 1)}
    got = device_map(pts.astype(F32).reshape(G, N, 3), labels.reshape(G, N), np.tile(IDENT, (G, 1)))

    live = np.ones(P, bool)
    live[dead] = False
    root = live.copy()
    root[[b for _, b in pairs]] = False
    ids = np.cumsum(root) - 1                                     # of a root: the roots before it
    n_roots, n_live = int(root.sum()), int(live.sum())
    assert got["num"].tolist() == [n_roots, n_live] == [P - 263 - 2, P - 263]
    node = np.where(root, ids, -1).astype(np.int32)
    for a, b in pairs:
        node[b] = ids[a]
    assert got["node_landmark"].tobytes() == node.reshape(G, N).tobytes()
    r = np.flatnonzero(root)
    center, count, spread = pts[r].copy(), np.ones(n_roots, np.int32), np.zeros(n_roots)
    for a, _ in pairs:
        center[ids[a], 0] += 0.25                                 # the mean of x and x + 0.5: exact
        count[ids[a]] = 2
        spread[ids[a]] = 0.25                                     # sqrt of the mean of 0.25^2, 0.25^2
    want = {"center": center, "label": labels[r], "count": count, "first": r.astype(np.int32),
            "sessions": np.ones(n_roots, np.int64), "spread": spread}
    for a, b in pairs:                                            # the planted pairs and their neighbours, by name first
        for i in (a - 1, a, b + 1):
            for name in want:
                assert got[name][ids[i]].tobytes() == want[name][ids[i]].tobytes(), (name, i)
    for name in want:
        assert got[name][:n_roots].tobytes() == want[name].tobytes(), name
        assert (got[name][n_roots:].view(np.uint8) == 0xFF).all(), name + ": written past the records"


# ------------------------------------------------------------------ labels and dead nodes
def test_labels_and_dead_nodes():
    rng = np.random.default_rng(11)
    G, N = 12, 16
    centers = rng.uniform(-2.0, 2.0, size=(G, N, 3)).astype(F32)
    labels = rng.integers(-3, 7, size=(G, N)).astype(np.int32)     # n_labels = 5: 5 and 6 are out of range
    labels[0, 0] = 0x7fffffff
    labels[0, 1] = -0x80000000
    radius = [0.75, 0.0, 0.75, 1.5, 0.3]                            # label 1 takes no part
    poses = np.tile(IDENT, (G, 1))
    poses[2, 0] = np.nan                                            # dead scans
    poses[3, 3] = np.inf
    poses[4, 1] = -np.inf
    centers[5, 3, 0] = np.nan                                       # dead nodes
    centers[5, 4, 2] = np.nan
    centers[5, 5, 1] = np.inf
    centers[6, :, 2] = F32(3e38)                                    # a height beyond the limit
    poses[7] = (1.0, 0.0, 2.0 ** 38, 0.0)                           # a coordinate beyond the limit
    poses[8] = (1.0, 0.0, 0.0, -(2.0 ** 37) - 1e5)
    poses[9] = (1.0, 0.0, 2.0 ** 36, -(2.0 ** 36))                  # ... and far out but inside it
    want = check(centers, labels, poses, radius=radius, n_labels=5)
    nl = want["node_landmark"]
    assert (nl[[2, 3, 4, 6, 7, 8]] == -1).all() and (nl[9][(labels[9] >= 0) & (labels[9] < 5) & (labels[9] != 1)] >= 0).all()
    assert (nl[labels == 1] == -1).all() and (nl[labels >= 5] == -1).all() and (nl[labels < 0] == -1).all()
    assert nl[5, 3] == nl[5, 4] == nl[5, 5] == -1 and 0 < want["num"][0] < want["num"][1]


# ------------------------------------------------------------------ capacity
def test_capacity(worlds):
    w = worlds[0]
    sub = slice(0, 20)
    args = (w["centers"][sub], w["labels"][sub], w["truth"][sub])
    found = int(ref.landmark_map(*args)["num"][0])
    assert found > 3
    for cap in (0, 1, found - 1, found, found + 5):
        want = check(*args, max_landmarks=cap)
        assert want["num"][0] == found and want["label"].shape[0] == min(cap, found)


# ------------------------------------------------------------------ sessions
def test_sixty_four_sessions_with_empty_and_one_scan_sessions():
    rng = np.random.default_rng(3)
    G, N = 70, 3
    starts = np.sort(np.concatenate(([0, 0, 1, 2, 2, 2], rng.integers(3, G + 1, size=58)))).astype(np.int32)
    assert starts.size == 64
    centers = rng.uniform(-1.5, 1.5, size=(G, N, 3)).astype(F32)
    centers[..., 2] = 0
    labels = rng.integers(0, 2, size=(G, N)).astype(np.int32)
    want = check(centers, labels, np.tile(IDENT, (G, 1)), starts=starts)
    seen = int(np.bitwise_or.reduce(want["sessions"]))
    assert bin(seen).count("1") > 20 and seen >> 32 != 0 and (want["count"] > 1).any()
    assert any(bin(int(v)).count("1") > 1 for v in want["sessions"])


# ------------------------------------------------------------------ order
def test_scan_order_decides_nothing(worlds):
    w = worlds[0]
    G, N = w["labels"].shape
    perm = np.random.default_rng(9).permutation(G)
    a = device_map(w["centers"], w["labels"], w["truth"])
    b = device_map(w["centers"][perm], w["labels"][perm], w["truth"][perm])
    assert a["num"].tolist() == b["num"].tolist()
    L = int(a["num"][0])
    old_of_new = a["node_landmark"][perm]                         # node (g', n) of b is node (perm[g'], n) of a
    live = b["node_landmark"] >= 0
    assert ((old_of_new >= 0) == live).all()
    pairs = np.unique(np.stack((b["node_landmark"][live], old_of_new[live]), axis=1), axis=0)
    assert pairs.shape[0] == L and np.unique(pairs[:, 0]).size == L and np.unique(pairs[:, 1]).size == L
    nb, na = pairs[:, 0], pairs[:, 1]
    for name in ("center", "spread", "count", "label"):
        assert b[name][nb].tobytes() == a[name][na].tobytes(), name


# ------------------------------------------------------------------ streams
def test_two_streams_two_dirty_workspaces(worlds):
    w = worlds[1]
    outs = [device_map(w["centers"], w["labels"], w["odom"], starts=w["starts"], stream=torch.cuda.Stream()) for _ in range(2)]
    for name in outs[0]:
        assert outs[0][name].tobytes() == outs[1][name].tobytes(), name


# ------------------------------------------------------------------ the Python layer
def test_build_reruns_when_the_capacity_is_too_small(worlds):
    from sg_pr_amd import landmarks
    w = worlds[0]
    want = ref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"])
    for cap in (3, None):
        lm = landmarks.build(w["centers"], w["labels"], w["truth"], starts=w["starts"], max_landmarks=cap)
        assert lm["num_landmarks"] == want["num"][0] and lm["live_nodes"] == want["num"][1]
        for name in ("center", "label", "count", "first", "sessions", "spread", "node_landmark"):
            assert lm[name].cpu().numpy().tobytes() == want[name].tobytes(), name
    short = torch.empty(landmarks.workspace_bytes(300, 100) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception, match="workspace"):
        landmarks.build_async(w["centers"], w["labels"], w["truth"], workspace=short)
    keep = landmarks.select(lm, min_count=3, min_sessions=2).cpu().numpy()
    bits = np.array([bin(int(v)).count("1") for v in want["sessions"]])
    assert (keep == ((want["count"] >= 3) & (bits >= 2))).all() and keep.any() and not keep.all()


def test_virtual_scans_agree_with_a_numpy_rendering(worlds):
    from sg_pr_amd import landmarks
    w = worlds[0]
    lm = landmarks.build(w["centers"], w["labels"], w["truth"], starts=w["starts"])
    keep = landmarks.select(lm, min_count=3)
    poses = w["truth"][200:300:7]
    for nn, rng_m in ((100, 50.0), (20, 30.0)):
        c, l = landmarks.virtual_scans(lm, poses, sensor_range=rng_m, node_num=nn, keep=keep)
        wc, wl = ref.virtual_scans(lm["center"].cpu().numpy(), lm["label"].cpu().numpy(), poses, rng_m, nn, keep.cpu().numpy())
        assert c.dtype == torch.float32 and l.dtype == torch.int32 and c.is_cuda
        assert (l.cpu().numpy() == wl).all() and (wl >= 0).sum() > 10 * len(poses)
        assert (wl[:, -1] == -1).any() if nn == 100 else (wl[:, -1] >= 0).any()      # padding; the cap
        # (float64 sums rounded to float32: one float32 ulp of a 50 m coordinate)
        assert np.abs(c.cpu().numpy() - wc).max() <= 4e-6


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
    """verify the world's true closures, select, optimise, map: the optimised map is nearer the true-pose map than the
    odometry's - fewer landmarks than the geometric mean of the two, more shared ones than their arithmetic mean"""
    from sg_pr_amd import metrics
    w = worlds[0]
    rows, cols = w["rows"].astype(np.int64), w["cols"].astype(np.int64)
    ver = model.verify_closures(w["centers"][rows], w["labels"][rows], cols[:, None], min_inliers=12,
                                col_centers=w["centers"], col_labels=w["labels"])
    sel = model.consistent_closures(ver, rows[:, None], cols[:, None], w["odom"], row_sessions=w["starts"],
                                    col_sessions=w["starts"])
    X, info = model.optimize_map(sel, ver, rows[:, None], cols[:, None], w["odom"], sessions=w["starts"])
    lm = model.landmark_map(w["centers"], w["labels"], X, sessions=w["starts"])
    want = ref.landmark_map(w["centers"], w["labels"], X.cpu().numpy(), starts=w["starts"])
    for name in ("center", "label", "count", "first", "sessions", "spread", "node_landmark"):
        assert lm[name].cpu().numpy().tobytes() == want[name].tobytes(), name
    opt = metrics.map_sharpness(lm)
    odo_lm = model.landmark_map(w["centers"], w["labels"], w["odom"], sessions=w["starts"])
    odo = metrics.map_sharpness(odo_lm)
    tru_lm = ref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"])
    tru = metrics.map_sharpness(tru_lm)
    n_opt, n_odo, n_tru = lm["num_landmarks"], odo_lm["num_landmarks"], int(tru_lm["num"][0])
    print("landmarks: optimised %d, odometry %d, true poses %d; shared %.3f / %.3f / %.3f; sharpness %.3f / %.3f / %.3f; "
          "closures accepted %d of %d"
          % (n_opt, n_odo, n_tru, opt["shared"], odo["shared"], tru["shared"], opt["sharpness"], odo["sharpness"],
             tru["sharpness"], int(sel["accept"].sum()), rows.size))
    assert n_opt < math.sqrt(n_odo * n_tru)
    assert opt["shared"] > 0.5 * (odo["shared"] + tru["shared"])



def test_place_db_landmarks_cli(model, tmp_path, ckpt_path, capsys):
    """--landmarks alone: the file holds the reference's map of the sequence on its own poses, the line its figures"""
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
    place_db.main([str(cfg), "--window", "30", "--landmarks", "--lm-radius", "0.8", "--lm-tau-z", "0.7"])
    line = next(l for l in capsys.readouterr().out.splitlines() if "landmark map of" in l)
    z = np.load(tmp_path / "eva" / "07_landmarks.npz")
    want = ref.landmark_map(centers, labels, metrics.planar_odometry(poses), radius=0.8, tau_z=0.7)
    for name in ("center", "label", "count", "first", "spread", "node_landmark"):
        assert z[name].tobytes() == want[name].tobytes(), name
    assert z["sessions"].view(np.uint64).tolist() == want["sessions"].tolist() and z["keep"].all()
    fig = metrics.map_sharpness(want)
    assert "landmarks %d sharpness %.4f m shared %.4f single %.4f" % (fig["landmarks"], fig["sharpness"], fig["shared"],
                                                                       fig["single"]) in line
    assert "of %d nodes" % want["num"][1] in line and "before" not in line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--landmarks", "--lm-radius", "0"])
