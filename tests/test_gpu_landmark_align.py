"""The alignment of scans to a landmark map on the GPU (sgpr_landmark_align, include/sgpr_landmark_align.h, DESIGN.md
§31): poses, node_landmark, stat and rms equal to the NumPy definition (tests/landmark_align_ref.py) to the bit - at the
shapes where the launch and a lane's slot count change, at landmark counts from none to several table sizes, at every
boundary of the association and the keep rule - then order-freedom, aliasing,
streams, the Python layer, the pipeline end to end and the command line.  Every output and the workspace are pre-filled
with 0xFF, and the outputs carry a margin that must stay 0xFF."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as ref  # noqa: E402
import landmark_ref as lref  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
MARGIN = 5
IDENT = (1.0, 0.0, 0.0, 0.0)


def device_align(centers, labels, poses, lm_center, lm_label, lm_use=None, radius=0.75, tau_z=0.75, iters=10, min_nodes=6,
                 n_labels=None, stream=None, in_place=False, ws_fill=0xFF, out_fill=0xFF, workspace=None):
    """the C call with every output (and a margin behind it) full of the byte out_fill and the workspace full of ws_fill
    (a given workspace is used as it is) -> dict of host arrays"""
    from sg_pr_amd import engine, landmarks
    lib = landmarks.load_library()
    dev = torch.device("cuda", 0)
    lab = torch.as_tensor(np.ascontiguousarray(labels, np.int32)).to(dev)
    Q, N = lab.shape
    cen = torch.as_tensor(np.ascontiguousarray(centers, F32).reshape(Q, N, 3)).to(dev)
    lmc = torch.as_tensor(np.ascontiguousarray(lm_center, np.float64).reshape(-1, 3)).to(dev)
    lml = torch.as_tensor(np.ascontiguousarray(lm_label, np.int32).reshape(-1)).to(dev)
    L = lml.numel()
    use = None if lm_use is None else torch.as_tensor(np.ascontiguousarray(lm_use, np.uint8).reshape(L)).to(dev)
    rad = np.atleast_1d(np.asarray(radius, np.float64))
    if rad.size == 1:
        rad = np.full(12 if n_labels is None else n_labels, rad[0])
    rad = np.ascontiguousarray(rad)

    def dirty(n, dtype):
        return torch.full((n * dtype.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(dtype)

    out = {"poses": dirty(4 * (Q + MARGIN), torch.float64), "node_landmark": dirty(Q * N + MARGIN, torch.int32),
           "stat": dirty(4 * (Q + MARGIN), torch.int32), "rms": dirty(Q + MARGIN, torch.float64)}
    X = torch.as_tensor(np.ascontiguousarray(poses, np.float64).reshape(Q, 4)).to(dev)
    if in_place:
        out["poses"][:4 * Q] = X.reshape(-1)
        X = out["poses"]
    need = landmarks.align_workspace_bytes(Q, N, L)
    assert need == ref.workspace_bytes(Q, N, L)
    ws = torch.full((max(need, 1),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs and the fills were made on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_landmark_align(p(cen), p(lab), Q, N, p(X), p(lmc) if L else None, p(lml) if L else None, p(use), L,
                                     rad.ctypes.data, rad.size, float(tau_z), int(iters), int(min_nodes), p(out["poses"]),
                                     p(out["node_landmark"]), p(out["stat"]), p(out["rms"]), p(ws), need, engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, Q, N, out_fill=0xFF):
    """the outputs equal the reference to the bit (NaN as NaN: bytes), nothing written past them"""
    for name, n in (("poses", 4 * Q), ("node_landmark", Q * N), ("stat", 4 * Q), ("rms", Q)):
        assert got[name][:n].tobytes() == want[name].tobytes(), (name, got[name][:n], want[name].reshape(-1))
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"


def check(centers, labels, poses, lm_center, lm_label, **kw):
    stream, in_place = kw.pop("stream", None), kw.pop("in_place", False)
    extra = {k: kw.pop(k) for k in ("ws_fill", "out_fill", "workspace") if k in kw}
    out_fill = extra.get("out_fill", 0xFF)
    got = device_align(centers, labels, poses, lm_center, lm_label, stream=stream, in_place=in_place, **extra, **kw)
    want = ref.align(centers, labels, poses, lm_center, lm_label, **kw)
    Q, N = np.asarray(labels).shape
    if Q * N == 0:                                               # nothing is written
        for name, v in got.items():
            tail = v[4 * Q:] if in_place and name == "poses" else v
            assert (tail.view(np.uint8) == out_fill).all(), name
        return want
    same(got, want, Q, N, out_fill)
    return want


def one(nodes, labels, pose, lm_center, lm_label, **kw):
    kw.setdefault("min_nodes", 2)
    return check(np.array([nodes], F32), np.array([labels], np.int32), np.array([pose], np.float64),
                 np.array(lm_center, np.float64).reshape(-1, 3), np.array(lm_label, np.int32), **kw)


def make_case(Q, N, L, seed, noise=0.1, perturb=0.15, labels=3, extent=None):
    """L landmarks of `labels` labels over a square, Q scans of N nodes that observe them from perturbed poses; one node
    in twenty is padding, one in twenty an object the map does not hold, one landmark in ten is not in use
    -> (centers, labels, poses, lm_center, lm_label, lm_use)"""
    rng = np.random.default_rng(seed)
    extent = extent if extent is not None else max(4.0, 1.5 * np.sqrt(max(L, 1)))
    Lp = max(L, 1)
    pts = np.concatenate((rng.uniform(-extent, extent, size=(Lp, 2)), rng.uniform(-1.0, 1.0, size=(Lp, 1))), axis=1)
    lm_label = rng.integers(0, labels, size=Lp)
    ids = rng.integers(0, Lp, size=(Q, N))
    yaw = rng.uniform(-3.0, 3.0, size=Q)
    t = rng.uniform(-5.0, 5.0, size=(Q, 2))
    d = pts[ids][..., :2] + rng.normal(0.0, noise, size=(Q, N, 2))
    new = rng.random((Q, N)) < 0.05
    d = np.where(new[..., None], rng.uniform(-extent, extent, size=(Q, N, 2)), d) - t[:, None, :]
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    centers = np.stack((c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0],
                        pts[ids][..., 2] + rng.uniform(-0.8, 0.8, size=(Q, N))), axis=-1)
    yaw = yaw + rng.normal(0.0, 0.05 * perturb, size=Q)
    t = t + rng.normal(0.0, perturb, size=(Q, 2))
    poses = np.stack((np.cos(yaw), np.sin(yaw), t[:, 0], t[:, 1]), axis=1)
    lab = np.where(rng.random((Q, N)) < 0.05, -1, lm_label[ids])
    use = (rng.random(Lp) < 0.9).astype(np.uint8)
    return centers.astype(F32), lab.astype(np.int32), poses, pts[:L], lm_label[:L].astype(np.int32), use[:L]


@pytest.fixture(scope="module")
def worlds():
    """seed -> the recipe of DESIGN.md §31: the map of drives 0 and 1 at the true poses, drive 2 displaced"""
    from sg_pr_amd import synth
    out = {}
    for seed in (0, 1):
        w = synth.landmark_world(seed)
        lm = lref.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=w["starts"][:2])
        rng = np.random.default_rng(500 + seed)
        start = synth._se2_compose(w["truth"][200:], synth._se2(rng.normal(0, 0.02, 100), rng.normal(0, 0.3, 100),
                                                                rng.normal(0, 0.3, 100)))
        out[seed] = {"w": w, "lm": lm, "use": (lm["count"] >= 3).astype(np.uint8), "start": start, "truth": w["truth"][200:],
                     "centers": w["centers"][200:], "labels": w["labels"][200:]}
    return out


# ------------------------------------------------------------------ shapes, landmark counts, iteration counts
@pytest.mark.parametrize("Q,N", [(1, 1), (1, 3), (2, 64), (3, 65), (5, 130), (17, 100)])
def test_shapes(Q, N):
    *case, use = make_case(Q, N, 300, Q * 1000 + N)
    for T in (0, 1, 2, 7):
        want = check(*case, lm_use=use, iters=T, min_nodes=2)
        if Q * N >= 128 and T >= 1:
            assert (want["stat"][:, 2] >= 1).all() and (want["stat"][:, 0] > N // 2).all()


@pytest.mark.parametrize("L", [0, 1, 2, 40, 300, 512, 513, 3000])
def test_landmark_counts(L):
    """no landmark, one, two, and tables of 1024 slots (up to 512 landmarks) and more"""
    *case, use = make_case(5, 130, L, 77 + L)
    for T in (0, 2):
        want = check(*case, lm_use=use, iters=T, min_nodes=2)
        check(*case, lm_use=None, iters=T, min_nodes=2)
        if L >= 40:
            assert (want["stat"][:, 0] > 60).all() and (want["node_landmark"] == -2).any()
        if L == 0:
            assert (want["stat"][:, 0] == 0).all() and (want["node_landmark"] < 0).all()


def test_no_slots():
    *case, use = make_case(4, 0, 30, 5)
    check(*case, lm_use=use, iters=2)
    check(*case, lm_use=use, iters=2, in_place=True)


# ------------------------------------------------------------------ association
@pytest.mark.parametrize("L_pad", [0, 600])
def test_cells_borders_and_signs(L_pad):
    """landmarks on both sides of cell borders and on one, negative coordinates, 0 and -0; with L_pad further landmarks
    far away the same cases run in a fuller table (cell width 0.75075 at radius 0.75, 2.002 at radius 2)"""
    far = np.concatenate((np.random.default_rng(3).uniform(500.0, 600.0, size=(L_pad, 2)), np.zeros((L_pad, 1))), axis=1)
    for r in (0.75, 2.0):
        w = max(r * 1.001, 0.5)
        lm, nodes = [], []
        for kx in (-3, -1, 0, 1, 2):
            for ky in (-2, 0, 1):
                bx, by = kx * w, ky * w
                lm += [(bx - 1e-9, by + 0.3, 0.0), (bx + 1e-9, by + 0.31, 0.0), (bx, by, 0.0)]       # either side, and on it
                nodes += [(bx - 0.4 * r, by + 0.3, 0.0), (bx + 0.4 * r, by - 0.2 * r, 0.0), (bx + 0.9 * r, by + 0.1, 0.0),
                          (bx - 1e-7, by - 1e-7, 0.0)]
        lm += [(0.0, 0.0, 0.0), (-0.0, -0.0, 0.0), (-0.0, 0.3, 0.0)]
        nodes += [(0.0, -0.0, 0.0), (-0.0, 0.0, 0.0), (-r, 0.0, 0.0), (0.0, r, 0.0)]
        lm_all = np.concatenate((np.array(lm), far))
        for pose in (IDENT, (1.0, 0.0, -0.0, -0.0), (0.0, 1.0, 0.1, -0.2), (-1.0, 0.0, 1e-9, 0.0)):
            want = one(nodes, [0] * len(nodes), pose, lm_all, [0] * len(lm_all), radius=r, iters=0)
            assert pose != IDENT or (want["node_landmark"] >= 0).sum() > len(nodes) // 2
            one(nodes, [0] * len(nodes), pose, lm_all, [0] * len(lm_all), radius=r, iters=2)


@pytest.mark.parametrize("L", [300, 900])
def test_many_landmarks_at_one_point_and_one_cell(L):
    """L landmarks at one point: the lowest id in use wins; a label whose landmarks all fall into one cell"""
    lm = np.tile((3.2, -1.1, 0.2), (L, 1))
    use = np.ones(L, np.uint8)
    use[:7] = 0
    nodes = [(3.0, -1.0, 0.0), (3.3, -1.2, 0.5), (9.0, 9.0, 0.0)]
    want = one(nodes, [1, 1, 1], IDENT, lm, [1] * L, lm_use=use, radius=0.75, iters=0)
    assert want["node_landmark"].tolist() == [[7, 7, -2]]
    rng = np.random.default_rng(L)
    cell = np.concatenate((rng.uniform(0.76, 1.49, size=(L, 2)), np.zeros((L, 1))), axis=1)      # inside cell (1, 1) of width 0.75075
    centers = np.concatenate((rng.uniform(0.0, 2.2, size=(2, 100, 2)), np.zeros((2, 100, 1))), axis=2).astype(F32)
    want = check(centers, np.full((2, 100), 2, np.int32), np.array([IDENT, (1.0, 0.0, 0.05, 0.0)]), cell, np.full(L, 2, np.int32),
                 radius=0.75, iters=3, min_nodes=2)
    assert (want["stat"][:, 0] > 20).all()


@pytest.mark.parametrize("L_pad", [0, 600])
def test_gate_and_height_boundaries(L_pad):
    far = [(500.0 + i, 500.0, 0.0) for i in range(L_pad)]
    z = F32(0.75)
    up = np.nextafter(z, F32(1))
    lm = [(0.0, 0.0, 0.0), (-np.spacing(0.75), 100.0, 0.0), (20.0, 0.0, 0.0), (30.0, 0.0, 0.0), (39.5, 0.0, 0.0), (40.5, 0.0, 0.0),
          (50.5, 0.0, 0.0), (49.5, 0.0, 0.0)] + far
    nodes = [(0.75, 0.0, 0.0), (0.75, 100.0, 0.0), (20.0, 0.0, z), (30.0, 0.0, up), (40.0, 0.0, 0.0), (50.0, 0.0, 0.0), (20.0, 0.0, -z)]
    want = one(nodes, [0] * 7, IDENT, lm, [0] * len(lm), radius=0.75, tau_z=0.75, iters=0)
    # at r r; one ulp past it; |dz| at tau_z; one float32 ulp past it; midway goes to the lower id, whichever side
    assert want["node_landmark"].tolist() == [[0, -2, 2, -2, 4, 6, 2]]


@pytest.mark.parametrize("L_pad", [0, 600])
def test_ineligible_landmarks_dead_nodes_and_the_limit(L_pad):
    nan, inf, past = float("nan"), float("inf"), float(np.nextafter(2.0 ** 37, np.inf))
    far = [(500.0 + i, 500.0, 0.0) for i in range(L_pad)]
    radius = [0.75, 0.0, 0.75]
    lm = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, nan), (past, 0.0, 0.0),
          (0.0, 0.0, -past), (0.0, -inf, 0.0), (0.2, 0.0, 0.0), (0.15, 0.0, 0.0), (2.0 ** 37, 0.0, 0.0), (2.0 ** 36, 7.0, 0.0)] + far
    lm_label = [1, 3, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0] + [0] * L_pad
    use = np.ones(len(lm), np.uint8)
    use[10] = 0
    nodes = [(0.1, 0.0, 0.0), (0.1, 0.0, 0.0), (0.1, 0.0, 0.0), (0.1, 0.0, 0.0), (nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf),
             (3e38, 0.0, 0.0), (0.0, 0.0, 3e38), (0.1, 0.0, 0.0)]
    want = one(nodes, [0, 1, 3, -1, 0, 0, 0, 0, 0, 2], IDENT, lm, lm_label, lm_use=use, radius=radius, iters=0)
    assert want["node_landmark"].tolist() == [[9, -1, -1, -1, -1, -1, -1, -1, -1, -2]]
    # coordinates at 2^37, one ulp past it, and at 2^36 (ulp 2^-16: the cell coordinates there are 2^36 / w)
    for X, node, lab in ((2.0 ** 37, 11, 0), (past, -1, 0), (2.0 ** 36, 12, 0)):
        want = one([(0.0, 7.0 if X == 2.0 ** 36 else 0.0, 0.0), (-0.5, 7.0 if X == 2.0 ** 36 else 0.0, 0.0)], [lab] * 2,
                   (1.0, 0.0, X, 0.0), lm, lm_label, lm_use=use, radius=radius, iters=1)
        assert want["node_landmark"][0, 0] == node, X
    want = one([(0.0, 0.0, 0.0)], [0], (1.0, 0.0, -2.0 ** 37, -2.0 ** 37), lm, lm_label, radius=radius, iters=0)
    assert want["node_landmark"].tolist() == [[-2]]
    # an infinite radius is a radius: everything of the label is in range, one cell
    want = one(nodes[:2], [0, 0], IDENT, lm, lm_label, lm_use=use, radius=[inf, 0.0, 0.75], iters=0)
    assert want["node_landmark"].tolist() == [[9, 9]]


def test_non_finite_poses_and_payloads():
    *case, use = make_case(8, 70, 300, 13)
    poses = case[2]
    poses[1, 0] = np.nan
    poses[2, 3] = np.inf
    poses[3, 1] = -np.inf
    poses[4].view(np.uint64)[2] = 0xfff8000000abcdef
    want = check(*case, lm_use=use, iters=3, min_nodes=2)
    assert want["poses"][1:5].tobytes() == poses[1:5].tobytes() and (want["node_landmark"][1:5] == -1).all()
    assert want["stat"][1:5].tolist() == [[0, 0, 0, 1]] * 4 and (want["stat"][[0, 5, 6, 7], 3] == 0).all()
    check(*case, lm_use=use, iters=0, min_nodes=2, in_place=True)


# ------------------------------------------------------------------ order and aliasing
@pytest.mark.parametrize("L", [300, 3000])
def test_query_order_and_landmark_order_decide_nothing(L):
    centers, labels, poses, lmc, lml, use = make_case(17, 100, L, 5 + L)
    a = device_align(centers, labels, poses, lmc, lml, lm_use=use, iters=4)
    perm = np.random.default_rng(9).permutation(17)
    b = device_align(centers[perm], labels[perm], poses[perm], lmc, lml, lm_use=use, iters=4)
    assert a["poses"][:68].reshape(17, 4)[perm].tobytes() == b["poses"][:68].tobytes()
    assert a["node_landmark"][:1700].reshape(17, 100)[perm].tobytes() == b["node_landmark"][:1700].tobytes()
    assert a["stat"][:68].reshape(17, 4)[perm].tobytes() == b["stat"][:68].tobytes()
    assert a["rms"][:17][perm].tobytes() == b["rms"][:17].tobytes()
    # landmarks permuted (random positions: no exact ties): the same poses, the ids mapped through the permutation
    lp = np.random.default_rng(10).permutation(L)                 # new id j is old id lp[j]
    inv = np.argsort(lp)
    c = device_align(centers, labels, poses, lmc[lp], lml[lp], lm_use=use[lp], iters=4)
    assert c["poses"][:68].tobytes() == a["poses"][:68].tobytes() and c["rms"][:17].tobytes() == a["rms"][:17].tobytes()
    old = a["node_landmark"][:1700]
    assert c["node_landmark"][:1700].tolist() == np.where(old >= 0, inv[np.maximum(old, 0)], old).tolist()
    assert c["stat"][:68].tobytes() == a["stat"][:68].tobytes() and (old >= 0).sum() > 1000


@pytest.mark.parametrize("L", [300, 3000])
def test_poses_out_may_be_poses(L):
    *case, use = make_case(17, 100, L, 21)
    want = check(*case, lm_use=use, iters=5, in_place=True)
    assert (want["stat"][:, 2] == 5).all()


# ------------------------------------------------------------------ the keep rule
def test_min_nodes_at_the_count():
    centers, labels, poses, lmc, lml, use = make_case(4, 40, 300, 7)
    base = ref.align(centers, labels, poses, lmc, lml, lm_use=use, iters=0)
    n = int(base["stat"][2, 0])
    assert n >= 20
    for mn, moved in ((n - 1, True), (n, True), (n + 1, False)):
        want = check(centers, labels, poses, lmc, lml, lm_use=use, iters=2, min_nodes=mn)
        assert (want["poses"][2].tobytes() != poses[2].tobytes()) == moved, mn
        assert want["stat"][2, 2] >= 1 if moved else want["stat"][2].tolist()[2:] == [0, 2]
    # coincident matched nodes: h == 0, the pose is kept; a scan without a match keeps it too
    centers[1, :, :2] = centers[1, 0, :2]
    labels[3] = -1
    want = check(centers, labels, poses, lmc, lml, lm_use=use, iters=3, min_nodes=2)
    assert want["poses"][[1, 3]].tobytes() == poses[[1, 3]].tobytes() and want["stat"][[1, 3], 3].tolist() == [2, 2]
    assert want["stat"][3].tolist() == [0, 0, 0, 2] and want["stat"][0, 2] >= 1


# ------------------------------------------------------------------ the planted world
@pytest.mark.parametrize("seed", [0, 1])
def test_world(worlds, seed):
    p = worlds[seed]
    lm = (p["lm"]["center"], p["lm"]["label"])
    single = check(p["centers"], p["labels"], p["start"], *lm, lm_use=p["use"], radius=0.75, iters=10)
    wide = check(p["centers"], p["labels"], p["start"], *lm, lm_use=p["use"], radius=2.0, iters=10)
    sched = check(p["centers"], p["labels"], wide["poses"], *lm, lm_use=p["use"], radius=0.75, iters=10)

    def err(X):
        return np.hypot(X[:, 2] - p["truth"][:, 2], X[:, 3] - p["truth"][:, 3])
    before, after = err(p["start"]), err(sched["poses"])
    assert (after < 0.5 * np.median(before)).all() and np.median(after) < 0.2 * np.median(before)
    assert (err(single["poses"]) > 0.5).any()


def test_two_streams_two_dirty_workspaces():
    for L in (300, 3000):
        *case, use = make_case(17, 100, L, 6)
        outs = [device_align(*case, lm_use=use, iters=5, stream=torch.cuda.Stream()) for _ in range(2)]
        want = ref.align(*case, lm_use=use, iters=5)
        for o in outs:
            same(o, want, 17, 100)


# ------------------------------------------------------------------ the Python layer
def test_python_layer_and_a_short_workspace(worlds):
    from sg_pr_amd import landmarks
    p = worlds[0]
    w = p["w"]
    lm = landmarks.build(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=w["starts"][:2])
    use = landmarks.select(lm, min_count=3)
    host = {k: lm[k].cpu().numpy() for k in ("center", "label")}
    X, info = landmarks.align(p["centers"], p["labels"], p["start"], lm, use=use, radius=2.0, iters=4)
    want = ref.align(p["centers"], p["labels"], p["start"], host["center"], host["label"], lm_use=use.cpu().numpy(), radius=2.0,
                     iters=4)
    assert X.is_cuda and X.cpu().numpy().tobytes() == want["poses"].tobytes()
    assert info["rms"].tobytes() == want["rms"].tobytes() and info["node_landmark"].tobytes() == want["node_landmark"].tobytes()
    assert np.stack([info[k] for k in ("matched", "live", "steps", "flags")], axis=1).tolist() == want["stat"].tolist()
    every = landmarks.align_async(p["centers"], p["labels"], p["start"], lm, iters=1)
    want = ref.align(p["centers"], p["labels"], p["start"], host["center"], host["label"], iters=1)
    assert every["poses"].cpu().numpy().tobytes() == want["poses"].tobytes()
    assert every["stat"].cpu().numpy().tolist() == want["stat"].tolist()
    short = torch.empty(landmarks.align_workspace_bytes(100, 100, lm["num_landmarks"]) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception, match="workspace"):
        landmarks.align_async(p["centers"], p["labels"], p["start"], lm, workspace=short)
    none = landmarks.align_async(np.zeros((0, 100, 3), F32), np.zeros((0, 100), np.int32), np.zeros((0, 4)), lm)
    assert none["poses"].shape == (0, 4) and none["node_landmark"].shape == (0, 100)


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


def test_align_to_map_after_localize(model, worlds):
    """drive 2 localised in the map of drives 0 and 1 from its true closures (SG.localize: a consensus over scan-to-scan
    transforms), then aligned to the landmark map from those poses: the schedule is the reference's, call by call, and
    the median error after alignment is below the median before"""
    p = worlds[0]
    w = p["w"]
    rows = np.arange(200, 300)
    cols = np.stack([np.clip(rows - 200 + d, 0, 99) + 100 * s for s in (0, 1) for d in (-1, 0, 1)], axis=1)
    ver = model.verify_closures(w["centers"][rows], w["labels"][rows], cols, min_inliers=12, col_centers=w["centers"][:200],
                                col_labels=w["labels"][:200])
    loc = model.localize(ver, cols, w["truth"][:200], min_support=2)
    ok = loc["accept"].cpu().numpy()
    assert ok.sum() >= 50
    start = loc["pose"].cpu().numpy()[ok]
    lm = model.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], sessions=w["starts"][:2])
    from sg_pr_amd import landmarks
    keep = landmarks.select(lm, min_count=3)
    X, info = model.align_to_map(p["centers"][ok], p["labels"][ok], start, lm, keep=keep)
    Z = start
    for r in (2.0, 0.75):
        out = ref.align(p["centers"][ok], p["labels"][ok], Z, lm["center"].cpu().numpy(), lm["label"].cpu().numpy(),
                        lm_use=keep.cpu().numpy(), radius=r, iters=10, min_nodes=6)
        Z = out["poses"]
    assert X.cpu().numpy().tobytes() == Z.tobytes() and info["node_landmark"].tobytes() == out["node_landmark"].tobytes()
    assert info["accept"].tolist() == (out["stat"][:, 0] >= 6).tolist() and info["matched"].tolist() == out["stat"][:, 0].tolist()
    truth = p["truth"][ok]
    before = np.hypot(start[:, 2] - truth[:, 2], start[:, 3] - truth[:, 3])
    after = np.hypot(Z[:, 2] - truth[:, 2], Z[:, 3] - truth[:, 3])
    print("localised %d of 100; median error %.4f m -> %.4f m after alignment" % (ok.sum(), np.median(before), np.median(after)))
    assert np.median(after) < np.median(before)
    # KITTI rows are taken as optimize_map takes them; min_matched moves accept alone
    rows12 = np.zeros((int(ok.sum()), 12))
    rows12[:, 0], rows12[:, 2], rows12[:, 3], rows12[:, 11] = start[:, 0], start[:, 1], start[:, 2], start[:, 3]
    Y, info2 = model.align_to_map(p["centers"][ok], p["labels"][ok], rows12, lm, keep=keep, min_matched=1000)
    assert np.abs(Y.cpu().numpy() - Z).max() < 1e-6 and not info2["accept"].any()


def test_place_db_align_cli(model, tmp_path, ckpt_path, capsys):
    """--landmarks --align: the file holds the reference's schedule from the sequence's own poses against the reference's
    map on them, the line the figures of both"""
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
    place_db.main([str(cfg), "--window", "30", "--landmarks", "--align", "--align-radii", "1.5,0.75", "--align-iters", "4"])
    lines = capsys.readouterr().out.splitlines()
    own = metrics.planar_odometry(poses)
    m = lref.landmark_map(centers, labels, own)
    Z = own
    for r in (1.5, 0.75):
        out = ref.align(centers, labels, Z, m["center"], m["label"], radius=r, iters=4, min_nodes=6)
        Z = out["poses"]
    z = np.load(tmp_path / "eva" / "07_align.npz")
    assert z["poses"].tobytes() == Z.tobytes() and z["start"].tobytes() == own.tobytes()
    assert z["node_landmark"].tobytes() == out["node_landmark"].tobytes() and z["rms"].tobytes() == out["rms"].tobytes()
    assert z["matched"].tolist() == out["stat"][:, 0].tolist() and z["live"].tolist() == out["stat"][:, 1].tolist()
    assert z["radii"].tolist() == [1.5, 0.75] and int(z["iters"]) == 4 and z["accept"].tolist() == (out["stat"][:, 0] >= 6).tolist()
    err = metrics.localization_errors(Z, own)
    line = next(l for l in lines if "aligned to its landmark map" in l)
    assert "gates 1.5, 0.75 m x 4 iterations" in line
    assert "translation %.4f / %.4f m -> %.4f / %.4f m" % (0.0, 0.0, np.median(err["trans_m"]), np.percentile(err["trans_m"], 95)) in line
    assert "matched share %.4f" % np.median(out["stat"][:, 0] / np.maximum(out["stat"][:, 1], 1)) in line
    assert "unmatched live nodes %d" % int((out["node_landmark"] == -2).sum()) in line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--align"])
