"""The tracking of drives through a landmark map on the GPU (sgpr_landmark_track, include/sgpr_landmark_track.h,
DESIGN.md §34): poses, predictions, node_landmark, stat, rms and num equal to the NumPy definition
(tests/landmark_track_ref.py) to the bit - on the planted world with and without a blackout, at the slot counts where a
lane's share and the staging of a scan change, on every stage layout, at every rule of the definition - then the
equality of a stage with sgpr_landmark_align on the GPU, streams, the Python layer, SG.track_in_map and the command line.
Every output and the workspace are pre-filled with 0xFF, and the outputs carry a margin that must stay 0xFF."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_ref as lref  # noqa: E402
import landmark_track_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
MARGIN = 5
OUTPUTS = ("poses", "pred", "node_landmark", "stat", "rms", "num")


def device_track(centers, labels, odom, init, lm_center, lm_label, lm_use=None, starts=None, radii=(2.0, 0.75), n_reacquire=0,
                 tau_z=0.75, iters=10, min_nodes=6, min_matched=10, max_shift=np.inf, flags=0, n_labels=None, stream=None,
                 ws_fill=0xFF, out_fill=0xFF, workspace=None):
    """the C call with every output (and a margin behind it) full of the byte out_fill and the workspace full of ws_fill
    (a given workspace is used as it is); the inputs must come back as they went in -> dict of host arrays"""
    from sg_pr_amd import engine, landmarks
    lib = landmarks.load_library()
    dev = torch.device("cuda", 0)
    lab = torch.as_tensor(np.ascontiguousarray(labels, np.int32)).to(dev)
    Q, N = lab.shape
    rad = np.ascontiguousarray(ref.radius_table(radii, n_labels))
    table = None if starts is None else np.ascontiguousarray(starts, np.int32)
    n_tracks = 1 if table is None else table.size
    host = {"centers": np.ascontiguousarray(centers, F32).reshape(Q, N, 3), "odom": np.ascontiguousarray(odom, np.float64).reshape(Q, 4),
            "init": np.ascontiguousarray(init, np.float64).reshape(n_tracks, 4),
            "lm_center": np.ascontiguousarray(lm_center, np.float64).reshape(-1, 3),
            "lm_label": np.ascontiguousarray(lm_label, np.int32).reshape(-1)}
    L = host["lm_label"].size
    if lm_use is not None:
        host["lm_use"] = np.ascontiguousarray(lm_use, np.uint8).reshape(L)
    d = {k: torch.as_tensor(v).to(dev) for k, v in host.items()}

    def dirty(n, dtype):
        return torch.full((n * dtype.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(dtype)

    out = {"poses": dirty(4 * (Q + MARGIN), torch.float64), "pred": dirty(4 * (Q + MARGIN), torch.float64),
           "node_landmark": dirty(Q * N + MARGIN, torch.int32), "stat": dirty(4 * (Q + MARGIN), torch.int32),
           "rms": dirty(Q + MARGIN, torch.float64), "num": dirty(4 + MARGIN, torch.int32)}
    need = landmarks.track_workspace_bytes(Q, N, L, rad.shape[0])
    assert need == ref.workspace_bytes(Q, N, L, rad.shape[0])
    ws = torch.full((max(need, 1),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs and the fills were made on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_landmark_track(p(d["centers"]), p(lab), Q, N, p(d["odom"]), None if table is None else table.ctypes.data,
                                     0 if table is None else table.size, p(d["init"]), p(d["lm_center"]) if L else None,
                                     p(d["lm_label"]) if L else None, p(d.get("lm_use")), L, rad.ctypes.data, rad.shape[0],
                                     int(n_reacquire), rad.shape[1], float(tau_z), int(iters), int(min_nodes), int(min_matched),
                                     float(max_shift), int(flags), p(out["poses"]), p(out["pred"]), p(out["node_landmark"]),
                                     p(out["stat"]), p(out["rms"]), p(out["num"]), p(ws), need, engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    for k, v in host.items():                                    # no output overlaps an input: they are what they were
        assert d[k].cpu().numpy().tobytes() == v.tobytes(), k + " was written"
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, Q, N, out_fill=0xFF):
    """the outputs equal the reference to the bit (NaN as NaN: bytes), nothing written past them"""
    for name, n in (("poses", 4 * Q), ("pred", 4 * Q), ("node_landmark", Q * N), ("stat", 4 * Q), ("rms", Q), ("num", 4)):
        assert got[name][:n].tobytes() == want[name].tobytes(), (name, got[name][:n], want[name].reshape(-1))
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"


def check(d, **kw):
    """a drive of ref.hand_drive / a dict of its keys through the call and the reference"""
    kw.setdefault("min_nodes", 2)
    kw.setdefault("iters", 3)
    args = (d["centers"], d["labels"], d["odom"], kw.pop("init", d["init"]), kw.pop("lm", d["lm"]), kw.pop("lm_label", d["lm_label"]))
    stream = kw.pop("stream", None)
    extra = {k: kw.pop(k) for k in ("ws_fill", "out_fill", "workspace") if k in kw}
    out_fill = extra.get("out_fill", 0xFF)
    got = device_track(*args, stream=stream, **extra, **kw)
    want = ref.track(*args, **kw)
    Q, N = d["labels"].shape
    if Q * N == 0:                                               # nothing is written
        assert all((v.view(np.uint8) == out_fill).all() for v in got.values())
        return want
    same(got, want, Q, N, out_fill)
    return want


def cut(d, lo, hi):
    return {k: (v[lo:hi] if k in ("centers", "labels", "odom", "truth") else v) for k, v in d.items()}


@pytest.fixture(scope="module")
def world():
    """the recipe of DESIGN.md §34 on seed 0, the track cut to the 70 scans from scan 60 on: it starts from its true pose
    perturbed; `blackout` masks every landmark within 52 m of the 4 scans from scan 85 on"""
    p = ref.planted_drive(0)
    c = cut(p, 60, 130)
    rng = np.random.default_rng(7)
    c["init"] = ref.compose(c["truth"][0], ref.se2(rng.normal(0, 0.02), rng.normal(0, 0.3), rng.normal(0, 0.3)))[None]
    gap = p["truth"][85:89, 2:]
    dist = np.hypot(p["lm"]["center"][:, None, 0] - gap[None, :, 0], p["lm"]["center"][:, None, 1] - gap[None, :, 1]).min(1)
    c["blackout"] = (p["use"] * (dist > 52.0)).astype(np.uint8)
    return c


def world_args(w):
    return (w["centers"], w["labels"], w["odom"], w["init"], w["lm"]["center"], w["lm"]["label"])


# ------------------------------------------------------------------ the planted world
@pytest.mark.parametrize("blackout", [False, True])
def test_world(world, blackout):
    kw = dict(lm_use=world["blackout" if blackout else "use"], radii=(8.0, 2.0, 0.75), n_reacquire=1)
    got = device_track(*world_args(world), **kw)
    want = ref.track(*world_args(world), **kw)
    same(got, want, 70, 100)
    lost = (want["stat"][:, 3] & ref.LOST) != 0
    err = np.hypot(want["poses"][:, 2] - world["truth"][:, 2], want["poses"][:, 3] - world["truth"][:, 3])
    if blackout:
        again = np.flatnonzero((want["stat"][:, 3] & (ref.REACQUIRE | ref.LOST)) == ref.REACQUIRE)
        assert 5 <= lost.sum() <= 60 and again.size >= 1 and not lost[-5:].any() and err[-5:].max() < 0.2
        assert want["poses"][lost].tobytes() == want["pred"][lost].tobytes()
    else:
        assert not lost.any() and err.max() < 0.2 and want["num"].tolist() == [70, 0, 0, 1]


def test_track_tables_on_the_world(world):
    """tracks of 0, 1 and 70 scans - the first scan once more as a track of its own in front of the drive - and of 1, 1
    and 1"""
    init = np.stack([world["init"][0], ref.compose(world["truth"][0], ref.se2(0.01, 0.2, 0.1)), world["init"][0]])
    kw = dict(lm_use=world["use"], starts=[0, 0, 1], iters=4)
    args = tuple(np.concatenate((world[k][:1], world[k])) for k in ("centers", "labels", "odom")) + (init,) + world_args(world)[4:]
    want = ref.track(*args, **kw)
    same(device_track(*args, **kw), want, 71, 100)
    assert want["num"].tolist() == [71, 0, 0, 2] and want["pred"][:2].tobytes() == init[1:].tobytes()
    three = cut(world, 0, 3)
    init[1] = ref.compose(world["truth"][1], ref.se2(-0.01, 0.1, 0.2))
    init[2] = ref.compose(world["truth"][2], ref.se2(0.0, -0.2, 0.2))
    args = world_args(three)[:3] + (init,) + world_args(three)[4:]
    want = ref.track(*args, lm_use=world["use"], starts=[0, 1, 2])
    same(device_track(*args, lm_use=world["use"], starts=[0, 1, 2]), want, 3, 100)
    assert want["num"].tolist() == [3, 0, 0, 3] and want["pred"].tobytes() == init.tobytes()


# ------------------------------------------------------------------ shapes and stage layouts
@pytest.mark.parametrize("N", [1, 63, 64, 65, 100, 130, 256, 257, 300])
def test_slot_counts(N):
    """a lane's share changes at 64 and 128 slots; a scan is staged in the LDS up to 256 slots and read from global
    memory past that"""
    d = ref.hand_drive(Q=6, N=N, seed=N, labels=3)
    d["labels"][:, ::17] = -1                                    # padding among the slots
    want = check(d, starts=[0, 1], init=np.stack([d["init"][0], ref.compose(d["truth"][1], ref.se2(0.0, 0.1, 0.1))]),
                 min_matched=min(10, N // 2))
    if N >= 63:
        assert want["num"].tolist() == [6, 0, 0, 2] and (want["stat"][:, 2] == 6).all()


@pytest.mark.parametrize("n_stages,n_reacquire", [(1, 0), (2, 0), (2, 1), (4, 0), (4, 1), (4, 3)])
def test_stage_layouts(n_stages, n_reacquire):
    d = ref.hand_drive(Q=9, N=40, seed=3)
    d["labels"][3:5] = -1                                        # two scans that see nothing: lost, then re-acquired
    radii = (8.0, 4.0, 2.0, 0.75)[4 - n_stages:]
    for flags in (0, ref.START_LOST):
        want = check(d, radii=radii, n_reacquire=n_reacquire, flags=flags)
        fl = want["stat"][:, 3]
        assert (fl[3:5] & ref.LOST).all() and want["num"].tolist() == [7, 2, 2, 1]
        assert bool(fl[5] & ref.REACQUIRE) == (n_reacquire > 0) and bool(fl[0] & ref.REACQUIRE) == (n_reacquire > 0 and flags != 0)
        assert want["stat"][6, 2] == 3 * (n_stages - n_reacquire) and want["stat"][5, 2] == 3 * n_stages


def test_no_iterations_and_few_landmarks():
    d = ref.hand_drive(Q=5, N=70, seed=5)
    want = check(d, iters=0)
    assert (want["stat"][:, 2] == 0).all() and want["poses"].tobytes() == want["pred"].tobytes()
    none = dict(lm=np.zeros((0, 3)), lm_label=np.zeros(0, np.int32))
    want = check(d, radii=(8.0, 2.0, 0.75), n_reacquire=1, **none)
    assert want["num"].tolist() == [0, 5, 5, 1] and (want["node_landmark"] == -2).all()
    assert check(d, min_matched=0, **none)["num"].tolist() == [5, 0, 0, 1]
    want = check(d, lm=d["lm"][:1], lm_label=d["lm_label"][:1], min_matched=1)
    assert (want["stat"][:, 0] == 1).all() and (want["stat"][:, 3] == ref.KEPT).all()


def test_use_mask_radius_zero_and_per_stage_radii():
    d = ref.hand_drive(Q=5, N=66, seed=6, labels=3)
    use = np.ones(66, np.uint8)
    use[::4] = 0
    base = check(d)                                              # lm_use NULL
    masked = check(d, lm_use=use)
    assert (base["stat"][:, 0] == 66).all() and (masked["stat"][:, 0] < 66).all()
    # label 1 takes no part in any stage; label 2 only in the wide one: eligible under THAT stage's radii
    want = check(d, radii=([2.0, 0.0, 2.0], [0.75, 0.0, 0.0]), n_labels=3)
    assert (want["stat"][:, 1] == 22).all() and (want["node_landmark"][:, 1::3] == -1).all()
    want = check(d, radii=([0.0, 0.0, 2.0], [0.75, 0.75, 0.75], [0.75, 0.0, np.inf]), n_reacquire=1, n_labels=3, flags=ref.START_LOST)
    assert (want["stat"][:, 1] == 44).all()


def test_non_finite_odometry_and_init():
    d = ref.hand_drive(Q=12, N=40, seed=8)
    d["odom"][3, 2] = np.nan
    d["odom"][7, 1] = np.inf
    init = np.stack([d["init"][0], d["init"][0], ref.compose(d["truth"][9], ref.se2(0.0, 0.1, 0.0))])
    init[1, 0] = np.nan
    init[1].view(np.uint64)[3] = 0xfff8000000abcdef
    want = check(d, init=init, starts=[0, 5, 9])
    assert want["stat"][:, 3].tolist() == [0, 0, 0, 8, 8] + [1] * 4 + [0] * 3 and want["num"].tolist() == [8, 0, 0, 3]
    assert want["poses"][5:9].tobytes() == np.tile(init[1], (4, 1)).tobytes()
    d["odom"][10] = np.nan
    check(d, init=init, starts=[0, 5, 9], max_shift=0.3)


def test_max_shift_finite_and_infinite():
    d = ref.hand_drive(Q=8, N=40, seed=9)
    free = check(d, max_shift=np.inf)
    assert free["num"][1] == 0
    shift = np.hypot(free["poses"][:, 2] - free["pred"][:, 2], free["poses"][:, 3] - free["pred"][:, 3])
    assert shift[0] > 0.2 and shift[1:].max() < 0.1
    want = check(d, max_shift=0.1)                               # the first scan is lost, the track never recovers the 0.25 m
    assert want["stat"][0, 3] & ref.LOST
    want = check(d, max_shift=0.1, radii=(8.0, 2.0, 0.75), n_reacquire=1)
    assert want["num"][1] >= 1
    assert check(d, max_shift=0.0)["num"].tolist() == [0, 8, 8, 1]


# ------------------------------------------------------------------ a stage is an alignment; streams; the Python layer
def test_a_one_scan_track_is_the_alignment_chained_on_the_gpu(world):
    from sg_pr_amd import landmarks
    one = cut(world, 0, 1)
    got = device_track(*world_args(one), lm_use=world["use"], radii=(8.0, 2.0, 0.75), n_reacquire=0)
    lm = {"center": torch.as_tensor(world["lm"]["center"]).cuda(), "label": torch.as_tensor(world["lm"]["label"]).cuda()}
    X, steps = world["init"], 0
    for r in (8.0, 2.0, 0.75):
        X, info = landmarks.align(one["centers"], one["labels"], X, lm, use=world["use"], radius=r, iters=10, min_nodes=6)
        steps += int(info["steps"][0])
    assert got["poses"][:4].tobytes() == X.cpu().numpy().tobytes() and got["pred"][:4].tobytes() == world["init"].tobytes()
    assert got["node_landmark"][:100].tobytes() == info["node_landmark"].tobytes() and got["rms"][:1].tobytes() == info["rms"].tobytes()
    assert got["stat"][:4].tolist() == [int(info["matched"][0]), int(info["live"][0]), steps, 0] and steps == 30


def test_two_streams_two_dirty_workspaces(world):
    w = cut(world, 0, 12)
    kw = dict(lm_use=world["blackout"], radii=(8.0, 2.0, 0.75), n_reacquire=1, starts=[0, 4, 8],
              init=np.stack([w["init"][0]] + [ref.compose(w["truth"][j], ref.se2(0.0, 0.1, -0.1)) for j in (4, 8)]))
    init = kw.pop("init")
    args = world_args(w)[:3] + (init,) + world_args(w)[4:]
    outs = [device_track(*args, stream=torch.cuda.Stream(), **kw) for _ in range(2)]
    want = ref.track(*args, **kw)
    for o in outs:
        same(o, want, 12, 100)


def test_python_layer_and_a_short_workspace(world):
    from sg_pr_amd import landmarks
    w = cut(world, 0, 20)
    lm = {"center": world["lm"]["center"], "label": world["lm"]["label"]}
    X, info = landmarks.track(w["centers"], w["labels"], w["odom"], w["init"], lm, use=world["blackout"], iters=4)
    want = ref.track(*world_args(w), lm_use=world["blackout"], radii=(8.0, 2.0, 0.75), n_reacquire=1, iters=4)
    assert X.is_cuda and X.cpu().numpy().tobytes() == want["poses"].tobytes() and info["pred"].tobytes() == want["pred"].tobytes()
    assert info["rms"].tobytes() == want["rms"].tobytes() and info["node_landmark"].tobytes() == want["node_landmark"].tobytes()
    assert np.stack([info[k] for k in ("matched", "live", "steps", "flags")], axis=1).tolist() == want["stat"].tolist()
    assert info["lost"].tolist() == ((want["stat"][:, 3] & ref.LOST) != 0).tolist() and info["num"].tolist() == want["num"].tolist()
    out = landmarks.track_async(w["centers"], w["labels"], w["odom"], w["init"], lm, radii=[[2.0] * 12, 0.75], reacquire_radii=None,
                                start_lost=True, max_shift=0.5)
    want = ref.track(*world_args(w), radii=(2.0, 0.75), max_shift=0.5, flags=ref.START_LOST)
    assert all(out[k].cpu().numpy().tobytes() == want[k].tobytes() for k in OUTPUTS)
    short = torch.empty(landmarks.track_workspace_bytes(20, 100, lm["label"].size, 3) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception, match="workspace"):
        landmarks.track_async(w["centers"], w["labels"], w["odom"], w["init"], lm, workspace=short)
    with pytest.raises(Exception, match="n_stages"):
        landmarks.track_async(w["centers"], w["labels"], w["odom"], w["init"], lm, radii=(4.0, 3.0, 2.0, 1.0))
    none = landmarks.track_async(np.zeros((0, 100, 3), F32), np.zeros((0, 100), np.int32), np.zeros((0, 4)), w["init"], lm)
    assert none["poses"].shape == (0, 4) and none["num"].tolist() == [0, 0, 0, 0]


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


def test_track_in_map_end_to_end(model, world):
    """the map of drives 0 and 1 built on the GPU, the cut of drive 2 tracked through its landmarks with three or more
    observations from KITTI rows: the reference on the same map, and a drive that follows the truth"""
    from sg_pr_amd import landmarks, synth
    w = synth.landmark_world(0, scans=300)
    lm = model.landmark_map(w["centers"][:600], w["labels"][:600], w["truth"][:600], sessions=w["starts"][:2])
    keep = landmarks.select(lm, min_count=3)
    rows = np.zeros((70, 12))
    rows[:, 0], rows[:, 2], rows[:, 3], rows[:, 11] = (world["odom"][:, j] for j in range(4))
    X, info = model.track_in_map(world["centers"], world["labels"], rows, world["init"], lm, use=keep)
    host = {k: lm[k].cpu().numpy() for k in ("center", "label")}
    own = ref.track(world["centers"], world["labels"], world["odom"], world["init"], host["center"], host["label"],
                    keep.cpu().numpy(), radii=(8.0, 2.0, 0.75), n_reacquire=1)
    assert np.abs(X.cpu().numpy() - own["poses"]).max() < 1e-6 and info["num"].tolist() == own["num"].tolist() == [70, 0, 0, 1]
    planar = model.track_in_map(world["centers"], world["labels"], world["odom"], world["init"], lm, use=keep)
    assert planar[0].cpu().numpy().tobytes() == own["poses"].tobytes() and planar[1]["node_landmark"].tobytes() == own["node_landmark"].tobytes()
    err = np.hypot(own["poses"][:, 2] - world["truth"][:, 2], own["poses"][:, 3] - world["truth"][:, 3])
    assert err.max() < 0.2 and not info["lost"].any()
    assert "localize" in model.track_in_map.__doc__ and "update_map" in model.track_in_map.__doc__


def test_place_db_track_cli(model, tmp_path, ckpt_path, capsys):
    """--landmarks --sessions 3 --track: the file holds the reference's track of the last session from its stored pose
    through the reference's map of the first two, the line the figures of both"""
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
    place_db.main([str(cfg), "--window", "30", "--landmarks", "--sessions", "3", "--track", "--track-radii", "1.5,0.75",
                   "--reacquire-radii", "6", "--min-matched", "12", "--align-iters", "4"])
    lines = capsys.readouterr().out.splitlines()
    own = metrics.planar_odometry(poses)
    m = lref.landmark_map(centers[:60], labels[:60], own[:60], starts=[0, 30])
    want = ref.track(centers[60:], labels[60:], own[60:], own[60:61], m["center"], m["label"], radii=(6.0, 1.5, 0.75), n_reacquire=1,
                     iters=4, min_nodes=6, min_matched=12)
    z = np.load(tmp_path / "eva" / "07_track.npz")
    assert z["poses"].tobytes() == want["poses"].tobytes() and z["pred"].tobytes() == want["pred"].tobytes()
    assert z["node_landmark"].tobytes() == want["node_landmark"].tobytes() and z["rms"].tobytes() == want["rms"].tobytes()
    assert np.stack([z[k] for k in ("matched", "live", "steps", "flags")], axis=1).tolist() == want["stat"].tolist()
    assert z["num"].tolist() == want["num"].tolist() and z["lost"].tolist() == ((want["stat"][:, 3] & ref.LOST) != 0).tolist()
    assert z["radii"].tolist() == [1.5, 0.75] and z["reacquire_radii"].tolist() == [6.0] and int(z["iters"]) == 4
    assert int(z["first_scan"]) == 60 and int(z["session"]) == 2 and not z["from_localize"] and z["init"].tobytes() == own[60:61].tobytes()
    line = next(l for l in lines if "tracked through the landmark map" in l)
    assert "session 2 of 3" in line and "gates 1.5, 0.75 m (after a lost scan 6 m first) x 4 iterations" in line
    assert "tracked %d, lost %d of 30 scans (fewer than 12 matches), longest lost run %d" % tuple(want["num"][:3]) in line
    assert "matched share %.4f" % np.median(want["stat"][:, 0] / np.maximum(want["stat"][:, 1], 1)) in line
    assert not os.path.exists(tmp_path / "eva" / "07_align.npz")
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--landmarks", "--track"])
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--landmarks", "--sessions", "3", "--track", "--track-radii", "4,3,2,1", "--reacquire-radii", "8"])
