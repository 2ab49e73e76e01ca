"""The alignment of scans to a landmark map (sgpr_landmark_align, include/sgpr_landmark_align.h) without
a GPU: the C-ABI surface of the sixth header and its argument checks, the NumPy definition
(tests/landmark_align_ref.py) on hand-made cases at every boundary of its rules and on synth.landmark_world - a map of two
drives, the third drive aligned to it from displaced poses: the conditions that make the stage worth having - and mutants
of the definition that must each change an output."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as ref  # noqa: E402
import landmark_ref as lref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
IDENT = (1.0, 0.0, 0.0, 0.0)
F32 = np.float32
SQUARE = [(1.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (-1.0, -1.0, 0.0), (1.0, -1.0, 0.0)]


def se2(yaw, x, y):
    return (math.cos(yaw), math.sin(yaw), x, y)


def one(nodes, labels, pose, lm_center, lm_label, **kw):
    """one scan through the reference"""
    kw.setdefault("min_nodes", 2)
    return ref.align(np.array([nodes], F32), np.array([labels], np.int32), np.array([pose], np.float64),
                     np.array(lm_center, np.float64).reshape(-1, 3), np.array(lm_label, np.int32), **kw)


# ------------------------------------------------------------------ C-ABI surface
def test_sixth_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, landmarks, localize, posegraph
    text = open(os.path.join(REPO, "include", "sgpr_landmark_align.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_landmark_align_workspace_bytes", "sgpr_landmark_align"] \
        == landmarks.ALIGN_ABI_SYMBOLS
    assert abi.constants == {} and abi.errors == {}
    lib = landmarks.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    (_, r0, a0), (_, r1, a1) = abi.functions
    assert r0 is ctypes.c_size_t and a0 == [ctypes.c_int] * 3
    assert r1 is ctypes.c_int and len(a1) == 21
    assert [a1[i] for i in (2, 3, 8, 10, 12, 13)] == [ctypes.c_int] * 6
    assert a1[11] is ctypes.c_double and a1[19] is ctypes.c_size_t
    assert all(a1[i] is ctypes.c_void_p for i in (0, 1, 4, 5, 6, 7, 9, 14, 15, 16, 17, 18, 20))
    # the build lists, and the other five headers are what they were
    assert "sgpr_landmark_align.hip" in _build.SOURCES and "sgpr_landmark_refine.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_landmark_align.h")) for h in _build.HEADERS[1:-1])
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any("align" in n for n in engine.ABI_SYMBOLS)
    assert landmarks.ABI_SYMBOLS == ["sgpr_landmark_workspace_bytes", "sgpr_landmark_map"]
    assert landmarks.REFINE_ABI_SYMBOLS == ["sgpr_landmark_refine_workspace_bytes", "sgpr_landmark_refine"]
    assert len(posegraph.ABI_SYMBOLS) == 2 and localize.ABI_SYMBOLS == ["sgpr_localize_scans"]
    assert (landmarks.ALIGN_NONFINITE, landmarks.ALIGN_KEPT) == (ref.NONFINITE, ref.KEPT) == (1, 2)


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import landmarks
    lib = landmarks.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    big = 1 << 40
    radius = (ctypes.c_double * 12)(*([0.75] * 12))

    def call(centers=g, labels=g, Q=8, N=10, poses=g, lmc=g, lml=g, use=g, L=20, rad=radius, n_labels=12, tau_z=0.75, iters=3,
             min_nodes=6, out=g, node=g, stat=g, rms=g, ws=g, wsb=big):
        return lib.sgpr_landmark_align(centers, labels, Q, N, poses, lmc, lml, use, L, rad, n_labels, tau_z, iters, min_nodes,
                                       out, node, stat, rms, ws, wsb, None)

    def says(word):
        return b"sgpr_landmark_align" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("centers", "labels", "poses", "lmc", "lml", "out", "node", "stat", "rms", "ws"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(rad=None) == INVALID and says("h_radius")
    assert call(Q=-1) == INVALID and says("Q ") and call(N=-1) == INVALID and says("N ")
    assert call(L=-1) == INVALID and says("L ") and call(iters=-1) == INVALID and says("iters")
    for mn in (1, 0, -5):
        assert call(min_nodes=mn) == INVALID and says("min_nodes"), mn
    for nl in (0, -1, 65):
        assert call(n_labels=nl) == INVALID and says("n_labels"), nl
    for bad in (-0.5, float("nan")):
        r = (ctypes.c_double * 12)(*([0.75] * 5 + [bad] + [0.75] * 6))
        assert call(rad=r) == INVALID and says("radius of label 5")
        assert call(tau_z=bad) == INVALID and says("tau_z")
    assert call(Q=1 << 16, N=1 << 15) == INVALID and says("int32")
    assert call(Q=0x7fffffff, N=0x7fffffff) == INVALID and says("int32")
    need = lib.sgpr_landmark_align_workspace_bytes(8, 10, 20)
    assert need > 0 and call(wsb=need - 1) == INVALID and says("workspace") and call(wsb=0) == INVALID and says("workspace")
    # Q == 0 or N == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    none = dict(centers=None, labels=None, poses=None, lmc=None, lml=None, use=None, out=None, node=None, stat=None, rms=None,
                ws=None, wsb=0)
    assert call(Q=0) == 0 and call(N=0) == 0 and call(Q=0, **none) == 0 and call(N=0, **none) == 0
    assert call(Q=0, min_nodes=1) == INVALID and call(N=0, iters=-2) == INVALID and call(Q=0, L=-1) == INVALID
    assert call(Q=0, rad=None) == INVALID and call(N=0, n_labels=0) == INVALID


def test_workspace_formula():
    from sg_pr_amd import landmarks
    for Q, N, L in ((1, 1, 0), (1, 1, 1), (2, 64, 11), (100, 100, 111), (300, 100, 512), (300, 100, 513), (4541, 100, 60000),
                    (4541, 100, 300000), (0, 100, 5), (7, 0, 5), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1 << 16, 1 << 15, 1),
                    (0x7fffffff, 1, 7)):
        assert landmarks.align_workspace_bytes(Q, N, L) == ref.workspace_bytes(Q, N, L), (Q, N, L)
    # a label and a list link per landmark, 12 bytes per slot of a table of at least 1024 and at least 2 L slots
    assert ref.workspace_bytes(1, 1, 0) == 1024 * 12 and ref.workspace_bytes(100, 100, 111) == 2 * 512 + 1024 * 12
    assert ref.workspace_bytes(9, 9, 513) == 2 * 2304 + 2048 * 12 and ref.workspace_bytes(1, 1, 7) % 256 == 0


# ------------------------------------------------------------------ the rules, on hand-made cases
def test_a_displaced_square_converges_in_one_step():
    yaw, tx, ty = 0.05, 0.2, -0.1
    c, s = math.cos(yaw), math.sin(yaw)
    truth = np.array(se2(yaw, tx, ty))
    lm = [(c * x - s * y + tx, s * x + c * y + ty, z) for x, y, z in SQUARE]
    out = one(SQUARE, [0] * 4, IDENT, lm, [0] * 4, radius=0.75, iters=1)
    assert out["node_landmark"].tolist() == [[0, 1, 2, 3]] and out["stat"].tolist() == [[4, 4, 1, 0]]
    assert np.abs(out["poses"][0] - truth).max() < 1e-12 and out["rms"][0] < 1e-12
    # T == 0: the association and the residual of the input, the input's bits
    out = one(SQUARE, [0] * 4, IDENT, lm, [0] * 4, radius=0.75, iters=0)
    assert out["poses"].tobytes() == np.array([IDENT]).tobytes() and out["stat"].tolist() == [[4, 4, 0, 0]]
    assert abs(out["rms"][0] - math.sqrt(np.mean([(a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 for a, b in zip(lm, SQUARE)]))) < 1e-12
    # a second step changes next to nothing, and counts
    out = one(SQUARE, [0] * 4, IDENT, lm, [0] * 4, radius=0.75, iters=2)
    assert np.abs(out["poses"][0] - truth).max() < 1e-12 and out["stat"].tolist() == [[4, 4, 2, 0]]


def test_gate_at_the_radius_and_one_ulp_past_it():
    r = 0.75
    r2 = np.float64(r) * np.float64(r)
    # a node at (d, 0) with d d == r r exactly, the landmark at the origin: 0.75 is a float32 and 0.5625 is exact
    out = one([(0.75, 0.0, 0.0)], [0], IDENT, [(0.0, 0.0, 0.0)], [0], radius=r, iters=0)
    assert np.float64(0.75) * np.float64(0.75) == r2 and out["node_landmark"].tolist() == [[0]]
    assert out["rms"][0] == 0.75 and out["stat"].tolist() == [[1, 1, 0, 0]]
    # the landmark moved so that the distance is one ulp (of float64) past the radius
    out = one([(0.75, 0.0, 0.0)], [0], IDENT, [(-np.spacing(0.75), 0.0, 0.0)], [0], radius=r, iters=0)
    d = np.float64(0.75) + np.spacing(0.75)
    assert d * d > r2 and out["node_landmark"].tolist() == [[-2]] and out["stat"].tolist() == [[0, 1, 0, 0]]
    assert out["rms"].view(np.uint64).tolist() == [0x7ff8000000000000]


def test_height_at_tau_z_and_one_float32_ulp_past_it():
    z = F32(0.75)
    out = one([(0.0, 0.0, z)], [0], IDENT, [(0.0, 0.0, 0.0)], [0], radius=1.0, tau_z=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[0]]
    out = one([(0.0, 0.0, np.nextafter(z, F32(1)))], [0], IDENT, [(0.0, 0.0, 0.0)], [0], radius=1.0, tau_z=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[-2]]
    out = one([(0.0, 0.0, -z)], [0], IDENT, [(0.0, 0.0, 0.0)], [0], radius=1.0, tau_z=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[0]]
    # z takes no part in the distance
    out = one([(0.5, 0.0, 0.5)], [0], IDENT, [(0.0, 0.0, 0.0)], [0], radius=1.0, tau_z=0.75, iters=0)
    assert out["rms"][0] == 0.5


def test_midway_goes_to_the_lower_id_whichever_side_it_is_on():
    a, b = (-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)
    assert one([(0.0, 0.0, 0.0)], [0], IDENT, [a, b], [0, 0], radius=1.0, iters=0)["node_landmark"].tolist() == [[0]]
    assert one([(0.0, 0.0, 0.0)], [0], IDENT, [b, a], [0, 0], radius=1.0, iters=0)["node_landmark"].tolist() == [[0]]
    # a nearer one wins over a lower id
    out = one([(0.25, 0.0, 0.0)], [0], IDENT, [a, b], [0, 0], radius=1.0, iters=0)
    assert out["node_landmark"].tolist() == [[1]] and out["rms"][0] == 0.25


def test_two_nodes_on_one_landmark_and_labels_apart():
    lm = [(0.0, 0.0, 0.0), (5.0, 0.0, 0.0)]
    out = one([(0.1, 0.0, 0.0), (-0.1, 0.0, 0.0), (5.0, 0.1, 0.0)], [0, 0, 0], IDENT, lm, [0, 0], radius=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[0, 0, 1]] and out["stat"].tolist() == [[3, 3, 0, 0]]    # no one-to-one rule
    # the same place, another label: no match
    out = one([(0.1, 0.0, 0.0), (5.0, 0.1, 0.0)], [1, 0], IDENT, lm, [0, 0], radius=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[-2, 1]]
    out = one([(0.1, 0.0, 0.0), (5.0, 0.1, 0.0)], [1, 0], IDENT, lm, [0, 1], radius=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[-2, -2]]


def test_dead_nodes_and_ineligible_landmarks():
    lm = [(0.0, 0.0, 0.0)] * 2
    radius = [0.75, 0.0, 0.75]                                   # label 1 takes no part; labels 0..2 exist
    nodes = [(0.1, 0.0, 0.0)] * 5
    out = one(nodes, [0, 1, 2, 3, -1], IDENT, lm, [0, 2], radius=radius, iters=0)
    assert out["node_landmark"].tolist() == [[0, -1, 1, -1, -1]] and out["stat"].tolist() == [[2, 2, 0, 0]]
    # landmarks of a radius-0 label, of labels out of range, NaN / infinite / out-of-range centres are not eligible
    nan, inf, far = float("nan"), float("inf"), np.nextafter(2.0 ** 37, np.inf)
    lm = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, nan), (far, 0.0, 0.0),
          (0.0, 0.0, -far), (0.2, 0.0, 0.0)]
    out = one([(0.1, 0.0, 0.0)] * 2, [0, 1], IDENT, lm, [1, 3, -1, 0, 0, 0, 0, 0, 0], radius=radius, iters=0)
    assert out["node_landmark"].tolist() == [[8, -1]]
    assert ref.eligible(lm, [1, 3, -1, 0, 0, 0, 0, 0, 0], None, np.array(radius)).tolist() == [-1] * 8 + [0]
    # a landmark AT the limit is eligible, and a node at the limit is live
    out = one([(0.0, 0.0, 0.0)], [0], (1.0, 0.0, 2.0 ** 37, 0.0), [(2.0 ** 37, 0.0, 0.0)], [0], radius=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[0]]
    out = one([(0.0, 0.0, 0.0)], [0], (1.0, 0.0, far, 0.0), [(2.0 ** 37, 0.0, 0.0)], [0], radius=0.75, iters=0)
    assert out["node_landmark"].tolist() == [[-1]] and out["stat"].tolist() == [[0, 0, 0, 0]]
    # a mask of zeros, a mask of one, no landmarks at all
    lm = [(0.0, 0.0, 0.0), (0.05, 0.0, 0.0)]
    assert one(nodes[:1], [0], IDENT, lm, [0, 0], lm_use=[0, 0], iters=2)["node_landmark"].tolist() == [[-2]]
    assert one(nodes[:1], [0], IDENT, lm, [0, 0], lm_use=[0, 1], iters=0)["node_landmark"].tolist() == [[1]]
    assert one(nodes[:1], [0], IDENT, lm, [0, 0], lm_use=None, iters=0)["node_landmark"].tolist() == [[1]]
    out = one(nodes[:2], [0, -1], IDENT, np.zeros((0, 3)), [], iters=2)
    assert out["node_landmark"].tolist() == [[-2, -1]] and out["stat"].tolist() == [[0, 1, 0, ref.KEPT]]
    assert out["rms"].view(np.uint64).tolist() == [0x7ff8000000000000]


def test_keep_rule():
    far = se2(0.05, 0.2, -0.1)
    lm = SQUARE
    # three matched nodes: min_nodes at the count and one above it
    out = one(SQUARE[:3], [0] * 3, far, lm, [0] * 4, radius=0.75, iters=3, min_nodes=3)
    assert out["poses"].tobytes() != np.array([far]).tobytes() and out["stat"][0].tolist() == [3, 3, 3, 0]
    out = one(SQUARE[:3], [0] * 3, far, lm, [0] * 4, radius=0.75, iters=3, min_nodes=4)
    assert out["poses"].tobytes() == np.array([far]).tobytes() and out["stat"][0].tolist() == [3, 3, 0, ref.KEPT]
    assert out["rms"][0] > 0.1
    # coincident matched nodes: p' is exactly 0, the moments vanish, h == 0
    out = one([SQUARE[0]] * 4, [0] * 4, far, lm, [0] * 4, radius=0.75, iters=2)
    assert out["poses"].tobytes() == np.array([far]).tobytes() and out["stat"][0].tolist() == [4, 4, 0, ref.KEPT]
    # T == 0 never fits and never sets KEPT
    out = one(SQUARE[:1], [0], far, lm, [0] * 4, radius=0.75, iters=0, min_nodes=6)
    assert out["stat"][0].tolist() == [1, 1, 0, 0]


def test_non_finite_poses():
    nodes = np.array([SQUARE] * 4, F32)
    labels = np.zeros((4, 4), np.int32)
    X = np.array([IDENT, (np.nan, 0.0, 0.0, 0.0), (1.0, 0.0, np.inf, 0.0), (1.0, -np.inf, 0.0, 0.0)])
    X[1].view(np.uint64)[0] = 0xfff8000000abcdef                 # a NaN with a payload: the bits are copied
    out = ref.align(nodes, labels, X, np.array(SQUARE), np.zeros(4, np.int32), iters=2, min_nodes=2)
    assert out["poses"][1:].tobytes() == X[1:].tobytes() and out["poses"][0].tolist() == list(IDENT)
    assert out["node_landmark"][1:].tolist() == [[-1] * 4] * 3 and out["node_landmark"][0].tolist() == [0, 1, 2, 3]
    assert out["stat"][1:].tolist() == [[0, 0, 0, ref.NONFINITE]] * 3
    assert out["rms"].view(np.uint64)[1:].tolist() == [0x7ff8000000000000] * 3 and out["rms"][0] == 0.0


def test_scan_sum_is_the_partials_and_the_tree():
    rng = np.random.default_rng(1)
    v = rng.normal(size=(1, 130)) * 10.0 ** rng.integers(-8, 8, size=(1, 130))
    used = rng.random((1, 130)) < 0.8
    part = [0.0] * 64
    for n in range(130):
        if used[0, n]:
            part[n % 64] = part[n % 64] + v[0, n]
    h = 32
    while h:
        for i in range(h):
            part[i] = part[i] + part[i + h]
        h //= 2
    assert ref.scan_sum(v, used)[0] == part[0]
    # the rms of a scan is that sum: 130 nodes on one landmark
    nodes = np.zeros((130, 3), F32)
    nodes[:, 0] = rng.uniform(-0.5, 0.5, 130)
    nodes[:, 1] = rng.uniform(-0.5, 0.5, 130)
    labels = np.where(used[0], 0, -1)
    out = one(nodes, labels, IDENT, [(0.0, 0.0, 0.0)], [0], radius=1.0, iters=0)
    x, y = nodes[:, 0].astype(np.float64), nodes[:, 1].astype(np.float64)
    d2 = (x * x + y * y)[None, :]
    assert out["rms"][0] == np.sqrt(ref.scan_sum(d2, used)[0] / np.float64(used.sum()))
    assert out["rms"][0] != np.sqrt(ref.scan_sum(d2, used, "sequential")[0] / np.float64(used.sum()))


# ------------------------------------------------------------------ the conditions, on the reference alone
def planted(seed):
    """the recipe of DESIGN.md §31: the landmark map of drives 0 and 1 of synth.landmark_world(seed) at the true poses,
    its landmarks with three or more observations, the 100 scans of drive 2 from displaced poses"""
    from sg_pr_amd import synth
    w = synth.landmark_world(seed)
    lm = lref.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=w["starts"][:2], radius=0.75, tau_z=0.75)
    use = (lm["count"] >= 3).astype(np.uint8)
    rng = np.random.default_rng(500 + seed)
    truth = w["truth"][200:]
    start = synth._se2_compose(truth, synth._se2(rng.normal(0, 0.02, 100), rng.normal(0, 0.3, 100), rng.normal(0, 0.3, 100)))
    # the true object of a landmark: the object most of its observations belong to
    ids, members = w["node_id"][:200].reshape(-1), lm["node_landmark"].reshape(-1)
    obj = np.full(lm["count"].size, -1, np.int64)
    for i in np.flatnonzero(use):
        vals, cnt = np.unique(ids[members == i], return_counts=True)
        obj[i] = vals[np.argmax(cnt)]
    return {"w": w, "lm": lm, "use": use, "truth": truth, "start": start, "obj": obj, "centers": w["centers"][200:],
            "labels": w["labels"][200:], "node_id": w["node_id"][200:]}


def trans_err(X, truth):
    return np.hypot(X[:, 2] - truth[:, 2], X[:, 3] - truth[:, 3])


@pytest.fixture(scope="module")
def runs():
    out = {}
    for seed in range(4):
        p = planted(seed)
        args = (p["centers"], p["labels"])
        lm = (p["lm"]["center"], p["lm"]["label"], p["use"])
        p["single"] = ref.align(*args, p["start"], *lm, radius=0.75, iters=10, min_nodes=6)
        wide = ref.align(*args, p["start"], *lm, radius=2.0, iters=10, min_nodes=6)
        p["sched"] = ref.align(*args, wide["poses"], *lm, radius=0.75, iters=10, min_nodes=6)
        out[seed] = p
    return out


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_alignment_recovers_the_drive_and_tells_new_objects_from_known_ones(runs, seed):
    p = runs[seed]
    w, truth = p["w"], p["truth"]
    before, single, after = trans_err(p["start"], truth), trans_err(p["single"]["poses"], truth), trans_err(p["sched"]["poses"], truth)
    yaw = np.degrees(np.abs(np.arctan2(p["sched"]["poses"][:, 1] * truth[:, 0] - p["sched"]["poses"][:, 0] * truth[:, 1],
                                       p["sched"]["poses"][:, 0] * truth[:, 0] + p["sched"]["poses"][:, 1] * truth[:, 1])))
    node, stat = p["sched"]["node_landmark"], p["sched"]["stat"]
    share = stat[:, 0] / stat[:, 1]
    live = node != -1
    tr = w["transient_session"][np.where(p["node_id"] >= 0, p["node_id"], 0)]
    transient, permanent = live & (tr == 2), live & (tr == -1)
    unmatched_transient = (node[transient] == -2).mean()
    matched_permanent = (node[permanent] >= 0).mean()
    hit = node >= 0
    on_true = (p["obj"][node[hit]] == p["node_id"][hit]).mean()
    print("seed %d: landmarks in use %d; before %.3f / %.3f m (median / 95 %%); one call at 0.75 m: %.3f / %.2f m (median / max), "
          "%.2f below 0.1 m; gates 2.0, 0.75: %.3f / %.3f / %.3f m (median / 95 %% / max); yaw %.3f deg; matched share "
          "%.3f / %.3f (median / min); transients unmatched %.3f; permanent matched %.3f; on the true object %.4f; "
          "minus-two nodes %d"
          % (seed, int(p["use"].sum()), np.median(before), np.percentile(before, 95), np.median(single), single.max(),
             (single < 0.1).mean(), np.median(after), np.percentile(after, 95), after.max(), np.median(yaw), np.median(share),
             share.min(), unmatched_transient, matched_permanent, on_true, int((node == -2).sum())))
    assert (after < 0.5 * np.median(before)).all() and np.median(after) < 0.2 * np.median(before)
    assert (single > 0.5).any()                                  # what the schedule is for
    assert unmatched_transient > 0.5 and matched_permanent > 0.5
    assert on_true >= 0.98
    assert (stat[:, 3] == 0).all() and (stat[:, 2] == 10).all()


# ------------------------------------------------------------------ mutants of the definition
def test_mutants_change_an_output():
    assert set(ref.MUTANTS) >= {"ties_high", "dist3d", "sequential", "uncentred", "fused_map"}
    rng = np.random.default_rng(2)
    Q, N, L = 6, 70, 60
    pts = np.concatenate((rng.uniform(-20.0, 20.0, size=(L, 2)), rng.uniform(-1.0, 1.0, size=(L, 1))), axis=1)
    pts[1] = pts[0]                                              # two landmarks at one place: the tie rule decides
    ids = rng.integers(0, L, size=(Q, N))
    yaw, t = rng.uniform(-3, 3, size=Q), rng.uniform(-5, 5, size=(Q, 2))
    d = pts[ids][..., :2] + rng.normal(0, 0.1, size=(Q, N, 2)) - t[:, None, :]
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    centers = np.stack((c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0],
                        pts[ids][..., 2] + rng.uniform(-0.6, 0.6, size=(Q, N))), axis=-1).astype(F32)
    yaw = yaw + rng.normal(0, 0.01, size=Q)
    X = np.stack((np.cos(yaw), np.sin(yaw), t[:, 0] + rng.normal(0, 0.1, size=Q), t[:, 1] + rng.normal(0, 0.1, size=Q)), axis=1)
    args = (centers, np.zeros((Q, N), np.int32), X, pts, np.zeros(L, np.int32))
    base = ref.align(*args, radius=0.75, iters=2, min_nodes=2)
    assert (base["stat"][:, 0] > 50).all() and (base["stat"][:, 2] == 2).all() and (base["node_landmark"] == 0).any()
    assert not (base["node_landmark"] == 1).any()
    changed = {}
    for m in ref.MUTANTS:
        out = ref.align(*args, radius=0.75, iters=2, min_nodes=2, mutant=m)
        changed[m] = sorted(k for k in base if out[k].tobytes() != base[k].tobytes())
        # every mutant is an alignment all the same: it is the bits that tell them apart
        assert m == "uncentred" or np.abs(out["poses"] - base["poses"]).max() < 0.05, m
    assert all(changed.values()), changed
    assert "node_landmark" in changed["ties_high"] and "node_landmark" in changed["dist3d"]
    assert changed["fused_map"] and changed["sequential"] and "poses" in changed["uncentred"]
    again = ref.align(*args, radius=0.75, iters=2, min_nodes=2, mutant=None)
    assert all(again[k].tobytes() == base[k].tobytes() for k in base)
    with pytest.raises(ValueError):
        ref.align(*args, mutant="nope")
