"""sgpr_posegraph_optimize on the MI355X against tests/posegraph_ref.py, EQUAL to the bit in X_out, info and resid: maps
at the segment ends and at the chunk boundaries of the tree sum, session layouts with empty and one-scan sessions,
closure lists of every shape, fixed sets, stopping rules, a dirty workspace on two streams, SG.optimize_map end to end
and the place_db command line."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegraph_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def same(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    return got.dtype == want.dtype and got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes()


MARGIN = 5


def device_optimize(X, rows, cols, T, starts=None, fixed=None, weight=None, w_odo=None, w_clo=None, max_iters=1000, rel_tol=1e-9,
                    stream=None, ws_fill=0xFF, out_fill=0xFF, workspace=None):
    """the C call with every output (and a margin behind it) full of the byte out_fill and the workspace full of ws_fill
    (a given workspace is used as it is) -> dict of host arrays"""
    from sg_pr_amd import engine, posegraph
    lib = posegraph.load_library()
    dev = torch.device("cuda", 0)
    w_odo, w_clo = posegraph.W_ODO if w_odo is None else w_odo, posegraph.W_CLO if w_clo is None else w_clo
    x = torch.as_tensor(np.ascontiguousarray(X, np.float64).reshape(-1, 4)).to(dev)
    r, c = (torch.as_tensor(np.ascontiguousarray(v, np.int32).reshape(-1)).to(dev) for v in (rows, cols))
    t = torch.as_tensor(np.ascontiguousarray(T, np.float64).reshape(-1, 4)).to(dev)
    M, C = x.shape[0], r.numel()
    wgt = None if weight is None else torch.as_tensor(np.ascontiguousarray(weight, np.float64).reshape(C)).to(dev)
    fx = None if fixed is None else torch.as_tensor(np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8).reshape(M)).to(dev)
    table = engine._session_table(starts)

    def dirty(n, dtype):
        return torch.full((n * dtype.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(dtype)

    out = {"X_out": dirty(4 * (M + MARGIN), torch.float64), "info": dirty(8 + MARGIN, torch.int32),
           "resid": dirty(4 + MARGIN, torch.float64)}
    need = posegraph.workspace_bytes(M, C)
    ws = torch.full((max(need, 16),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs and the fills were made on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_posegraph_optimize(p(x), M, *engine._table_args(table), p(r), p(c), p(t), p(wgt), C, p(fx), float(w_odo[0]),
                                         float(w_odo[1]), float(w_clo[0]), float(w_clo[1]), int(max_iters), float(rel_tol),
                                         p(out["X_out"]), p(out["info"]), p(out["resid"]), p(ws), ws.numel(), engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_outputs(got, want, M, out_fill=0xFF):
    """device_optimize's outputs equal the reference's (X_out, info, resid) to the bit, nothing written past them"""
    for name, n, w in (("X_out", 4 * M, want[0]), ("info", 8, want[1]), ("resid", 4, want[2])):
        assert got[name][:n].tobytes() == np.ascontiguousarray(w).tobytes(), (name, got[name][:n], np.asarray(w).reshape(-1))
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"


def check(X, rows, cols, T, **kw):
    """the call against the reference -> the reference's (X_out, info, resid)"""
    from sg_pr_amd import posegraph
    rows, cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    T = np.asarray(T, np.float64).reshape(-1, 4)
    out, info, resid = posegraph.optimize_async(X, rows, cols, T, **kw)
    torch.cuda.synchronize()
    want = ref.optimize(X, rows, cols, T, **kw)
    assert same(info, want[1]), (info.cpu().tolist(), want[1].tolist())
    assert same(resid, want[2]), (resid.cpu().tolist(), want[2].tolist())
    assert same(out, want[0]), "X_out: %d of %d doubles differ, largest gap %.3g" % (
        int((out.cpu().numpy() != want[0]).sum()), want[0].size, float(np.abs(out.cpu().numpy() - want[0]).max()))
    return want


def loop_map(seed, lens, closures):
    """a stacked map of sessions of the given lengths (0 allowed), each a drifting walk in a frame of its own, and
    `closures` noisy closures between random scans at most 3 apart in walk position -> X, starts, rows, cols, T"""
    from sg_pr_amd import synth
    rng = np.random.default_rng(seed)
    n = max(max(lens), 1)
    heading, xy = synth._random_walk(rng, n)
    parts, walkpos = [], []
    for d, L in enumerate(lens):
        Xt = synth._se2(heading[:L] + rng.normal(0, 0.01, L), xy[:L, 0] + rng.normal(0, 0.1, L), xy[:L, 1] + rng.normal(0, 0.1, L))
        parts.append(synth._se2_compose(synth._se2(0.7 * d, 13.0 * d, -7.0 * d), Xt))
        walkpos.append(np.arange(L))
    X, walkpos = np.concatenate(parts), np.concatenate(walkpos)
    starts = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int32)
    M = X.shape[0]
    rows = rng.integers(0, M, size=closures)
    near = [np.nonzero((np.abs(walkpos - walkpos[r]) <= 3) & (np.arange(M) != r))[0] for r in rows]
    cols = np.array([rng.choice(c) if c.size else r for c, r in zip(near, rows)], dtype=np.int64).reshape(-1)
    sess = np.searchsorted(starts, np.arange(M), side="right") - 1
    frames = np.stack([synth._se2(0.7 * d, 13.0 * d, -7.0 * d) for d in range(len(lens))])
    true = synth._se2_compose(synth._se2_inverse(frames[sess]), X)             # every scan in the common frame
    T = synth._se2_compose(synth._se2(rng.normal(0, 0.01, closures), rng.normal(0, 0.1, closures), rng.normal(0, 0.1, closures)),
                           synth._se2_compose(synth._se2_inverse(true[cols]), true[rows]))
    return X, starts, rows.astype(np.int32), cols.astype(np.int32), np.ascontiguousarray(T.reshape(-1, 4))


@pytest.fixture(scope="module")
def world():
    from sg_pr_amd import synth
    return synth.drift_world(1)


# ------------------------------------------------------------------ 1. maps by size and session layout
def test_drift_world(world):
    from sg_pr_amd import metrics
    w = world
    out, info, _ = check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"])
    assert info[3] == info[4] == ref.CONVERGED and info[1] > 10 and info[2] > 10
    assert metrics.trajectory_error(out, w["truth"]) <= metrics.trajectory_error(w["odom"], w["truth"]) / 20.0


@pytest.mark.parametrize("lens", [(64, 64, 64), (65, 65, 65), (63,), (128, 1, 129)])
def test_segment_ends(lens):
    X, starts, rows, cols, T = loop_map(len(lens) * 100 + lens[0], lens, 40)
    info = check(X, rows, cols, T, starts=starts)[1]
    assert info[7] >= 1 and info[1] > 0 and info[2] > 0


@pytest.mark.parametrize("M", [1, 2, 1023, 1024, 1025, 2049])
def test_chunk_boundaries_of_the_tree_sum(M):
    lens = (M,) if M < 1000 else (M // 2, M - M // 2)
    X, starts, rows, cols, T = loop_map(M, lens, min(3 * M // 8, 200))
    if M == 2:
        rows, cols = np.array([1], np.int32), np.array([0], np.int32)          # parallel to the one odometry edge
        T = ref_rel(X, rows, cols) + np.array([[0.0, 0.001, 0.05, -0.02]])
    info = check(X, rows, cols, T, starts=starts, max_iters=60)[1]
    if M >= 1023:
        assert info[6] == M - 1 and info[1] > 5 and info[2] > 5


def test_sixty_four_sessions_with_empty_and_one_scan_sessions():
    lens = [(0, 1, 5, 70, 0, 0, 64, 1, 2, 33)[j % 10] for j in range(64)]
    X, starts, rows, cols, T = loop_map(64, lens, 400)
    assert starts.size == 64 and len(set(starts.tolist())) < 64
    check(X, rows, cols, T, starts=starts)                    # scan 0 is a one-scan session behind an empty one
    # the same map anchored in a late session, and in two places
    fixed = np.zeros(X.shape[0], bool)
    fixed[-1] = True
    info = check(X, rows, cols, T, starts=starts, fixed=fixed)[1]
    assert info[7] >= 8 and info[1] > 0 and info[2] > 0
    fixed[10] = True
    check(X, rows, cols, T, starts=starts, fixed=fixed)


# ------------------------------------------------------------------ 2. closure counts and shapes
@pytest.mark.parametrize("C", [0, 1, 65])
def test_closure_counts(C):
    X, starts, rows, cols, T = loop_map(C + 5, (70, 50), C)
    info = check(X, rows, cols, T, starts=starts)[1]
    assert info[5] <= C and (C > 0 or info[1:5].tolist() == [0, 0, 0, 0])


def test_duplicated_parallel_and_piled_up_closures():
    X, starts, rows, cols, T = loop_map(11, (90, 90), 60)
    # every closure three times, shuffled; then 65 closures on one scan; then closures along odometry edges, both ways
    rng = np.random.default_rng(0)
    perm = rng.permutation(180)
    r3, c3, T3 = np.tile(rows, 3)[perm], np.tile(cols, 3)[perm], np.tile(T, (3, 1))[perm]
    assert check(X, r3, c3, T3, starts=starts)[1][5] >= 170
    pile_r = np.full(65, 40, np.int32)
    pile_c = (100 + np.arange(65) % 7).astype(np.int32)
    pile_T = np.tile(T[:1], (65, 1)) + rng.normal(0, 0.01, (65, 4))
    check(X, np.concatenate((rows, pile_r, pile_c)), np.concatenate((cols, pile_c, pile_r)),
          np.concatenate((T, pile_T, pile_T)), starts=starts, weight=rng.uniform(0.5, 2.0, 190))
    k = np.array([10, 11, 50, 120], np.int32)
    rel = ref_rel(X, k + 1, k)
    check(X, np.concatenate((rows, k + 1, k)), np.concatenate((cols, k, k + 1)),
          np.concatenate((T, rel, ref_rel(X, k, k + 1))), starts=starts)


def ref_rel(X, rows, cols):
    from sg_pr_amd import synth
    return synth._se2_compose(synth._se2_inverse(X[cols]), X[rows])


def test_void_closures_of_every_kind():
    X, starts, rows, cols, T = loop_map(13, (60, 60), 40)
    M = X.shape[0]
    T = T.copy()
    weight = np.ones(40)
    rows[1], cols[2], rows[3], cols[4] = -1, -1, M, M
    cols[5] = rows[5]
    T[6, 0], T[7, 3], T[8, 1], T[9, 2] = np.nan, np.inf, -np.inf, np.nan
    T[10, :2] = 0.0
    weight[11], weight[12], weight[13], weight[14] = 0.0, -2.0, np.nan, np.inf
    out, info, _ = check(X, rows, cols, T, starts=starts, weight=weight)
    live = np.ones(40, bool)
    live[1:15] = False
    assert info[5] == live.sum()
    clean = ref.optimize(X, rows[live], cols[live], T[live], starts=starts)
    assert out.tobytes() == clean[0].tobytes()
    # every closure void: the input
    out, info, _ = check(X, rows[1:5], cols[1:5], T[1:5], starts=starts)
    assert info[5] == 0 and out.tobytes() == X.tobytes()


# ------------------------------------------------------------------ 3. fixed sets and status
def test_fixed_sets(world):
    w = world
    M = 600
    frozen = np.arange(M) < 300                                     # localise the second drive against a frozen map
    out, info, _ = check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"], fixed=frozen)
    assert info[6] == 300 and out[:300].tobytes() == w["odom"][:300].tobytes()
    out, info, _ = check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"], fixed=np.ones(M, bool))
    assert info[6] == 0 and info[1:5].tolist() == [0, 0, 0, 0] and out.tobytes() == w["odom"].tobytes()
    out, info, _ = check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"], fixed=np.zeros(M, bool))
    assert info.tolist() == [ref.NO_ANCHOR, 0, 0, 0, 0, 0, 0, 0] and out.tobytes() == w["odom"].tobytes()
    scattered = np.arange(M) % 37 == 5
    check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"], fixed=scattered)


def test_nonfinite_poses_return_the_input(world):
    w = world
    for k, j, v in ((0, 0, np.nan), (599, 3, np.inf), (301, 2, -np.inf)):
        X = w["odom"].copy()
        X[k, j] = v
        out, info, _ = check(X, w["rows"], w["cols"], w["T"], starts=w["starts"])
        assert info[0] == ref.NONFINITE
    X = w["odom"].copy()
    X[77, :2] = 0.0
    assert check(X, w["rows"], w["cols"], w["T"], starts=w["starts"], fixed=np.zeros(600, bool))[1][0] == 3


# ------------------------------------------------------------------ 4. stopping rules
def test_stopping_rules(world):
    w = world
    full = check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"])[1]
    for iters in (0, 1, int(full[1]) - 1):
        info = check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"], max_iters=iters)[1]
        assert info[1] == iters and info[3] == ref.STOP_MAX_ITERS
    info = check(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"], rel_tol=0.0, max_iters=200)[1]
    assert info[1] == 200 or info[3] != ref.STOP_MAX_ITERS


# ------------------------------------------------------------------ 5. workspace, streams, the Python surface
def test_dirty_workspace_on_two_streams(world):
    from sg_pr_amd import posegraph
    w = world
    want = ref.optimize(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"])
    need = posegraph.workspace_bytes(600, 120)
    X, T = torch.as_tensor(w["odom"]).cuda(), torch.as_tensor(w["T"]).cuda()
    rows, cols = torch.as_tensor(w["rows"]).cuda(), torch.as_tensor(w["cols"]).cuda()
    spaces = [torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    got = []
    for ws in spaces:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got.append(posegraph.optimize_async(X, rows, cols, T, starts=w["starts"], workspace=ws))
    torch.cuda.synchronize()
    for out, info, resid in got:
        assert same(out, want[0]) and same(info, want[1]) and same(resid, want[2])
    # a short workspace is refused
    with pytest.raises(Exception, match="workspace"):
        posegraph.optimize_async(X, rows, cols, T, starts=w["starts"], workspace=spaces[0][:need - 1])
    out, info = posegraph.optimize(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"])
    assert same(out, want[0]) and info["iterations"] == (int(want[1][1]), int(want[1][2]))
    assert info["stop"] == ("converged", "converged") and info["live_closures"] == 120 and info["status"] == 0


@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_optimize_map_end_to_end(model):
    """two 120-scan slices of one world as two sessions in unrelated frames: retrieved, verified, selected, optimised.
    Equality with the reference run on the accepted records, and the merged map lands on the truth."""
    import math
    from sg_pr_amd import metrics, synth
    centers, labels, _, poses = synth.world_sequence(360, 100, seed=6)
    a, b = slice(0, 120), slice(240, 360)
    pooled = model.embed(centers, labels)[0]
    vals, idx = model.loop_closures(pooled[b], pooled[a], k=1)
    ver = model.verify_closures(centers[b], labels[b], idx, values=vals, min_inliers=12, col_centers=centers[a],
                                col_labels=labels[a])
    rows = np.arange(120, dtype=np.int64)[:, None]
    frame = np.array([[math.cos(2.3), math.sin(2.3), -310.0, 95.0]])
    Xa, Xb = metrics.planar_odometry(poses[a]), metrics.planar_odometry(poses[b])
    Xb_own = synth._se2_compose(frame, Xb)
    sel = model.consistent_closures(ver, rows, idx, Xb_own, col_poses=Xa)
    out, info = model.optimize_map(sel, ver, rows, idx, Xa, row_poses=Xb_own)
    acc = sel["accept"].cpu().numpy().reshape(-1)
    assert acc.sum() >= 3 and info["session_starts"].tolist() == [0, 120]
    X = np.concatenate((Xa, Xb_own))
    want = ref.optimize(X, rows.reshape(-1)[acc] + 120, idx.cpu().numpy().reshape(-1)[acc],
                        ver["refined"].cpu().numpy().reshape(-1, 4)[acc], starts=[0, 120])
    assert same(out, want[0]) and (info["info"] == want[1]).all() and (info["resid"] == want[2]).all()
    assert info["live_closures"] == acc.sum() and info["free_scans"] == 239 and info["active_sessions"] == 2
    truth = np.concatenate((Xa, Xb))
    assert metrics.trajectory_error(X, truth) > 20.0 and metrics.trajectory_error(out, truth) < 1.0


def test_place_db_optimize_cli(model, tmp_path, ckpt_path, capsys):
    """--verify --consistent --optimize --save-poses: the file holds the reference's poses for the closures written"""
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
    saved = tmp_path / "poses.npy"
    place_db.main([str(cfg), "--k", "2", "--window", "30", "--verify", "--min-inliers", "15", "--consistent", "--sessions", "2",
                   "--max-trans", "0.8", "--max-yaw-deg", "3", "--lever-gain", "0.03", "--min-clique", "4", "--optimize",
                   "--save-poses", str(saved)])
    line = next(l for l in capsys.readouterr().out.splitlines() if "pose graph over" in l)
    z = np.load(tmp_path / "eva" / "07_consistent.npz")
    ok = z["consistent"]
    X = metrics.planar_odometry(poses)
    want = ref.optimize(X, z["rows"][ok], z["cols"][ok], z["refined"][ok], starts=[0, 75])
    got = np.load(saved)
    assert got.dtype == np.float64 and got.shape == (150, 4) and got.tobytes() == want[0].tobytes()
    assert "over %d closures" % want[1][5] in line and "iterations %d + %d" % (want[1][1], want[1][2]) in line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--verify", "--optimize"])
