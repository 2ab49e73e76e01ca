"""The landmark map (sgpr_landmark_map, include/sgpr_landmarks.h) without a GPU: the C-ABI surface of the
fourth header and its argument checks, the NumPy definition (tests/landmark_ref.py) on hand-made cases and on
synth.landmark_world - the conditions that make the stage worth having - mutants of the definition that must each change
an output, the virtual scans, the sharpness metric, and verification against the map measured with geo_ref."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_ref  # noqa: E402
import landmark_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
IDENT = (1.0, 0.0, 0.0, 0.0)
F32 = np.float32
CENTER_NOISE = 0.15


@pytest.fixture(scope="module")
def worlds():
    from sg_pr_amd import synth
    return [synth.landmark_world(seed) for seed in range(4)]


@pytest.fixture(scope="module")
def true_maps(worlds):
    return [ref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"]) for w in worlds]


def scene(points, labels, **kw):
    """one scan per point under identity poses, through the reference"""
    pts = np.asarray(points, F32).reshape(-1, 1, 3)
    return ref.landmark_map(pts, np.asarray(labels, np.int32).reshape(-1, 1), np.tile(IDENT, (pts.shape[0], 1)), **kw)


def popcount(words):
    return np.array([bin(int(v)).count("1") for v in np.asarray(words).reshape(-1)], dtype=np.int64)


# ------------------------------------------------------------------ C-ABI surface
def test_fourth_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, landmarks, localize, posegraph
    text = open(os.path.join(REPO, "include", "sgpr_landmarks.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_landmark_workspace_bytes", "sgpr_landmark_map"] == landmarks.ABI_SYMBOLS
    assert abi.constants == {"SGPR_LANDMARK_MAX_LABELS": 64} and landmarks.MAX_LABELS == 64 == ref.MAX_LABELS
    lib = landmarks.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    (_, r0, a0), (_, r1, a1) = abi.functions
    assert r0 is ctypes.c_size_t and a0 == [ctypes.c_int, ctypes.c_int]
    assert r1 is ctypes.c_int and len(a1) == 22
    assert [a1[i] for i in (2, 3, 6, 8, 10)] == [ctypes.c_int] * 5 and a1[9] is ctypes.c_double and a1[20] is ctypes.c_size_t
    assert all(a1[i] is ctypes.c_void_p for i in (0, 1, 4, 5, 7, 11, 12, 13, 14, 15, 16, 17, 18, 19, 21))
    # the build lists, and the other three headers are what they were
    assert "sgpr_landmarks.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_landmarks.h")) for h in _build.HEADERS[1:-1])
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any(n.startswith("sgpr_landmark") for n in engine.ABI_SYMBOLS)
    assert len(posegraph.ABI_SYMBOLS) == 2 and localize.ABI_SYMBOLS == ["sgpr_localize_scans"]


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import landmarks
    lib = landmarks.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    nan = float("nan")
    table = np.array([0, 4, 4, 8], np.int32)
    radius = np.full(12, 0.75)
    big = 1 << 40

    def call(centers=g, labels=g, G=8, N=10, poses=g, starts=None, ns=0, rad=radius, nl=12, tau_z=0.75, cap=80, center=g,
             label=g, count=g, first=g, sessions=g, spread=g, node=g, num=g, ws=g, wsb=big):
        s = None if starts is None else starts.ctypes.data
        r = None if rad is None else rad.ctypes.data
        return lib.sgpr_landmark_map(centers, labels, G, N, poses, s, ns, r, nl, tau_z, cap, center, label, count, first,
                                     sessions, spread, node, num, ws, wsb, None)

    def says(word):
        return b"sgpr_landmark_map" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("centers", "labels", "poses", "center", "label", "count", "first", "sessions", "spread", "node", "num", "ws"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(rad=None) == INVALID and says("NULL h_radius")
    assert call(G=-1) == INVALID and says("G ") and call(N=-1) == INVALID and says("N ")
    assert call(cap=-1) == INVALID and says("max_landmarks")
    for n in (0, -1, 65, 1 << 30):
        assert call(nl=n) == INVALID and says("n_labels"), n
    for bad in (-1e-9, -float("inf"), nan):
        r = radius.copy()
        r[7] = bad
        assert call(rad=r) == INVALID and says("radius of label 7"), bad
        assert call(tau_z=bad) == INVALID and says("tau_z"), bad
    # the session table
    assert call(starts=table, ns=0) == INVALID and says("session table")
    assert call(starts=None, ns=2) == INVALID and says("NULL session table")
    assert call(starts=table, ns=65) == INVALID and says("number of sessions")
    assert call(starts=table, ns=-1) == INVALID and says("number of sessions")
    assert call(starts=np.array([1, 4], np.int32), ns=2) == INVALID and says("start at 0")
    assert call(starts=np.array([0, 5, 4], np.int32), ns=3) == INVALID and says("decreasing")
    assert call(starts=np.array([0, 9], np.int32), ns=2) == INVALID and says("past 8")
    # node indices are int32
    assert call(G=1 << 16, N=1 << 15) == INVALID and says("int32")
    assert call(G=0x7fffffff, N=0x7fffffff) == INVALID and says("int32")
    # the workspace
    need = lib.sgpr_landmark_workspace_bytes(8, 10)
    assert call(wsb=need - 1) == INVALID and says("workspace") and call(wsb=0) == INVALID and says("workspace")
    # G == 0 or N == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    none = dict(centers=None, labels=None, poses=None, center=None, label=None, count=None, first=None, sessions=None,
                spread=None, node=None, num=None, ws=None, wsb=0)
    assert call(G=0) == 0 and call(N=0) == 0 and call(G=0, **none) == 0 and call(N=0, cap=0, **none) == 0
    assert call(G=0, starts=np.array([0, 0], np.int32), ns=2) == 0
    assert call(G=0, nl=0) == INVALID and call(N=0, tau_z=nan) == INVALID and call(G=0, rad=None) == INVALID
    assert call(G=0, starts=np.array([0, 1], np.int32), ns=2) == INVALID and says("past 0")


def test_workspace_formula():
    from sg_pr_amd import landmarks
    for G, N in ((1, 1), (2, 256), (2, 257), (300, 100), (4541, 100), (5 * 4541, 100), (0, 100), (7, 0), (-1, 5), (5, -1),
                 (1 << 16, 1 << 15), (0x7fffffff, 1)):
        assert landmarks.workspace_bytes(G, N) == ref.workspace_bytes(G, N), (G, N)
    P = 5 * 4541 * 100
    assert ref.workspace_bytes(5 * 4541, 100) >= 84 * P + 12 * 2 * P           # per-node arrays + a table of >= 2 P slots
    assert ref.workspace_bytes(1, 1) % 256 == 0 and ref.workspace_bytes(1, 1) >= 1024 * 12


# ------------------------------------------------------------------ the rules, on hand-made cases
def test_a_chain_is_one_landmark():
    lm = scene([(0, 0, 0), (0.7, 0, 0), (1.4, 0, 0)], [3, 3, 3])
    assert lm["num"].tolist() == [1, 3] and lm["count"].tolist() == [3] and lm["first"].tolist() == [0]
    assert lm["node_landmark"].reshape(-1).tolist() == [0, 0, 0] and lm["label"].tolist() == [3]
    assert scene([(0, 0, 0), (1.4, 0, 0)], [3, 3])["num"].tolist() == [2, 2]       # (a and c alone do not link)
    # the centre is the mean of the fixed-point coordinates, the spread the RMS planar distance to it
    x = [round(float(F32(v)) * ref.FIX) for v in (0.0, 0.7, 1.4)]
    cx = float(sum(x)) / (3.0 * ref.FIX)
    assert lm["center"][0].tolist() == [cx, 0.0, 0.0]
    q = sum(round(min((float(F32(v)) - cx) * (float(F32(v)) - cx), ref.D2_CAP) * ref.FIX) for v in (0.0, 0.7, 1.4))
    assert lm["spread"][0] == math.sqrt(float(q) / (3.0 * ref.FIX)) and abs(lm["spread"][0] - 0.7 * math.sqrt(2 / 3)) < 1e-6


def test_labels_radii_and_scans():
    lm = scene([(1, 1, 0), (1, 1, 0)], [2, 5])                    # equal places, different labels
    assert lm["num"].tolist() == [2, 2] and lm["label"].tolist() == [2, 5]
    radius = [0.75] * 12
    radius[4] = 0.0
    lm = scene([(0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), (0.1, 0.1, 0)], [4, 4, 6, 6], radius=radius)     # a radius-0 label
    assert lm["num"].tolist() == [1, 2] and lm["node_landmark"].reshape(-1).tolist() == [-1, -1, 0, 0]
    assert lm["first"].tolist() == [2]
    # labels outside 0..n_labels-1 are dead
    lm = scene([(0, 0, 0)] * 4, [-1, 12, 11, 0x7fffffff])
    assert lm["num"].tolist() == [1, 1] and lm["node_landmark"].reshape(-1).tolist() == [-1, -1, 0, -1]
    # two nodes of ONE scan in range link: there is no cannot-link rule
    pts = np.array([[(0, 0, 0), (0.5, 0, 0), (9, 9, 0)]], F32)
    lm = ref.landmark_map(pts, np.array([[1, 1, 1]], np.int32), [IDENT])
    assert lm["num"].tolist() == [2, 3] and lm["node_landmark"].tolist() == [[0, 0, 1]]
    # the height decides as well
    assert scene([(0, 0, 0), (0, 0, 0.75)], [0, 0])["num"][0] == 1 and scene([(0, 0, 0), (0, 0, 0.76)], [0, 0])["num"][0] == 2


def test_poses_sessions_and_the_limit():
    c, s = math.cos(0.5), math.sin(0.5)
    pts = np.array([[(2, 1, 0.25)], [(2, 1, 0.25)], [(0, 0, 0)], [(0, 0, 0)], [(0, 0, 0)]], F32)
    poses = np.array([IDENT, (c, s, 10.0, -3.0), (1, 0, 2.0 ** 37, 0), (1, 0, np.nextafter(2.0 ** 37, np.inf), 0),
                      (np.nan, 0, 0, 0)])
    lm = ref.landmark_map(pts, np.zeros((5, 1), np.int32), poses, starts=[0, 1, 1, 3])
    assert lm["node_landmark"].reshape(-1).tolist() == [0, 1, 2, -1, -1] and lm["num"].tolist() == [3, 3]
    # (one member: the centre is its map point on the 2^-24 m grid of the fixed point)
    grid = [float(round(v * ref.FIX)) / (1.0 * ref.FIX) for v in ((c * 2.0 - s * 1.0) + 10.0, (s * 2.0 + c * 1.0) + -3.0)]
    assert lm["center"][1].tolist() == grid + [0.25]
    assert lm["center"][2].tolist() == [2.0 ** 37, 0.0, 0.0]
    assert lm["sessions"].tolist() == [1, 4, 4]                   # session 1 is empty: scan 1 and 2 belong to session 2
    assert lm["spread"].tolist() == [0.0, 0.0, 0.0] and lm["count"].tolist() == [1, 1, 1]


# ------------------------------------------------------------------ the conditions, on the reference alone
def purity(w, lm):
    """(share of the landmarks with count >= 2 whose nodes are ONE true object, share of the true objects observed twice
    or more that lie in ONE landmark)"""
    live = lm["node_landmark"] >= 0
    pairs = np.unique(np.stack((lm["node_landmark"][live], w["node_id"][live]), axis=1), axis=0)
    objs_per_lm = np.bincount(pairs[:, 0], minlength=int(lm["num"][0]))
    n_obj = int(w["transient_session"].size)
    lms_per_obj = np.bincount(pairs[:, 1], minlength=n_obj)
    seen = np.bincount(w["node_id"][live], minlength=n_obj)
    return float(np.mean(objs_per_lm[lm["count"] >= 2] == 1)), float(np.mean(lms_per_obj[seen >= 2] == 1))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_recovers_the_planted_objects(worlds, true_maps, seed):
    from sg_pr_amd import metrics
    w, lm = worlds[seed], true_maps[seed]
    assert w["centers"].shape == (300, 100, 3) and w["starts"].tolist() == [0, 100, 200]
    assert (w["node_id"] >= 0).sum() == lm["num"][1] == (w["labels"] >= 0).sum()
    pure, whole = purity(w, lm)
    # which true object a landmark is: the object of its first member
    obj = w["node_id"].reshape(-1)[lm["first"]]
    transient = w["transient_session"][obj] >= 0
    seen_by = np.zeros((w["transient_session"].size, 3), bool)
    for d in range(3):
        seen_by[np.unique(w["node_id"][100 * d:100 * (d + 1)][w["labels"][100 * d:100 * (d + 1)] >= 0]), d] = True
    permanent = seen_by.all(1)[obj] & ~transient
    one = popcount(lm["sessions"]) == 1
    sharp = metrics.map_sharpness(lm)
    print("seed %d: %d landmarks of %d nodes, %d links; pure %.4f whole %.4f; one-session share: transients %.3f (%d), "
          "permanent %.3f (%d); sharpness %.4f = %.3f x noise sqrt 2; shared %.3f single %.3f"
          % (seed, lm["num"][0], lm["num"][1], lm["links"], pure, whole, one[transient].mean(), transient.sum(),
             one[permanent].mean(), permanent.sum(), sharp["sharpness"], sharp["sharpness"] / (CENTER_NOISE * math.sqrt(2)),
             sharp["shared"], sharp["single"]))
    assert pure >= 0.98 and whole >= 0.98
    assert transient.sum() >= 5 and permanent.sum() >= 20
    assert one[transient].mean() > 0.5 and one[permanent].mean() < 0.5
    assert 0.9 * CENTER_NOISE * math.sqrt(2) <= sharp["sharpness"] <= 1.2 * CENTER_NOISE * math.sqrt(2)


def rigid_fit(est, truth):
    """the planar rigid motion F (c, s, x, y) that fits the positions of F o est to those of truth in the least squares"""
    a, b = est[:, 2] + 1j * est[:, 3], truth[:, 2] + 1j * truth[:, 3]
    rot = np.vdot(a - a.mean(), b - b.mean())
    rot = rot / abs(rot)
    t = b.mean() - rot * a.mean()
    return np.array([rot.real, rot.imag, t.real, t.imag])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_drift_blunts_the_map(worlds, true_maps, seed):
    """every drive's odometry, put into the truth's frame by one rigid fit, maps less sharply than the true poses"""
    from sg_pr_amd import metrics, synth
    w = worlds[seed]
    aligned = np.concatenate([synth._se2_compose(rigid_fit(w["odom"][s:s + 100], w["truth"][s:s + 100])[None, :],
                                                 w["odom"][s:s + 100]) for s in w["starts"]])
    assert metrics.trajectory_error(aligned, w["truth"]) < 2.0 < metrics.trajectory_error(w["odom"], w["truth"])
    drift = metrics.map_sharpness(ref.landmark_map(w["centers"], w["labels"], aligned, starts=w["starts"]))
    true = metrics.map_sharpness(true_maps[seed])
    print("seed %d: sharpness %.4f at true poses, %.4f on aligned odometry (landmarks %d / %d)"
          % (seed, true["sharpness"], drift["sharpness"], true["landmarks"], drift["landmarks"]))
    assert drift["sharpness"] > true["sharpness"]


# ------------------------------------------------------------------ mutants of the definition
def differs(a, b):
    return any(np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() for k in a if k != "links")


def test_mutants_change_an_output(worlds, true_maps):
    assert len(ref.MUTANTS) >= 5 and {"strict", "dist3d", "fused_map", "float_sum", "ids_high"} <= set(ref.MUTANTS)
    w, base = worlds[0], true_maps[0]
    on_world = {m: differs(ref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"], mutant=m), base)
                for m in ("float_sum", "ids_high")}
    assert all(on_world.values()), on_world
    # a fused product in the map point: c x - s y cancels to exactly 0 when every product is rounded, and to the rounding
    # error of one product when the other is fused into the difference - enough to part two nodes at a tiny radius
    c = math.cos(math.pi / 4)
    x = float(F32(1.1))
    pts = np.array([[(x, x, 0)], [(0, 0, 0)]], F32)
    poses = np.array([(c, c, 0.0, 0.0), (1.0, 0.0, 0.0, c * x + c * x)])
    kw = dict(radius=1e-30)
    assert ref.map_points(pts, poses)[0, 0, 0] == 0.0 != ref.map_points(pts, poses, "fused_map")[0, 0, 0]
    assert abs(ref.map_points(pts, poses, "fused_map")[0, 0, 0]) < 1e-15
    assert ref.landmark_map(pts, np.zeros((2, 1), np.int32), poses, **kw)["num"][0] == 1
    assert ref.landmark_map(pts, np.zeros((2, 1), np.int32), poses, mutant="fused_map", **kw)["num"][0] == 2
    # a strict < on a 3-4-5 offset at radius 5; a strict height rule at |dz| == tau_z; 3-D distance where dz matters
    edge = ([(0, 0, 0), (3, 4, 0)], [0, 0])
    assert scene(*edge, radius=5.0)["num"][0] == 1 and scene(*edge, radius=5.0, mutant="strict")["num"][0] == 2
    high = ([(0, 0, 0), (0, 0, 0.75)], [0, 0])
    assert scene(*high)["num"][0] == 1 and scene(*high, mutant="z_strict")["num"][0] == 2
    both = ([(0, 0, 0), (0.6, 0, 0.6)], [0, 0])
    assert scene(*both)["num"][0] == 1 and scene(*both, mutant="dist3d")["num"][0] == 2
    # ids by the highest member: (0, 3) and (1, 2) swap
    pts = ([(0, 0, 0), (5, 0, 0), (5.1, 0, 0), (0.1, 0, 0)], [0] * 4)
    assert scene(*pts)["node_landmark"].reshape(-1).tolist() == [0, 1, 1, 0]
    assert scene(*pts, mutant="ids_high")["node_landmark"].reshape(-1).tolist() == [1, 0, 0, 1]
    # the definition itself, named as no mutant, is the base
    assert not differs(ref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"], mutant=None), base)
    with pytest.raises(ValueError):
        scene(*edge, mutant="nope")


# ------------------------------------------------------------------ virtual scans and the metric
def test_virtual_scans_on_a_hand_made_map():
    from sg_pr_amd import landmarks
    center = np.array([(50.0, 0, 0.5), (0, 50.000001, 0), (3, 0, -1), (0, 3, 1), (0, -3, 2), (-3, 0, 3), (1, 1, 0), (60, 60, 0)])
    lm = {"center": center, "label": np.array([5, 5, 9, 2, 2, 2, 0, 1], np.int32)}
    poses = np.array([IDENT, (0.0, 1.0, 0.0, 0.0), (1.0, 0.0, 100.0, 0.0)])
    c, l = landmarks.virtual_scans(lm, poses, sensor_range=50.0, node_num=8)
    c, l = c.numpy(), l.numpy()
    assert c.shape == (3, 8, 3) and c.dtype == np.float32 and l.dtype == np.int32
    # the range boundary: 50 m is in, a hair more is out; label order, stable: 0 | 2 2 2 in id order | 5 | 9; padding
    assert l[0].tolist() == [0, 2, 2, 2, 5, 9, -1, -1]
    assert c[0, :6].tolist() == [[1, 1, 0], [0, 3, 1], [0, -3, 2], [-3, 0, 3], [50, 0, 0.5], [3, 0, -1]]
    assert (c[0, 6:] == 0).all()
    # a pose rotated by 90 degrees: the map's +y is the sensor's forward, the map's +x its right
    assert l[1].tolist() == l[0].tolist()
    assert c[1, :6].tolist() == [[1, -1, 0], [3, 0, 1], [-3, 0, 2], [0, 3, 3], [0, -50, 0.5], [0, -3, -1]]
    # the third pose sees the one landmark 50 m behind it
    assert l[2].tolist() == [5] + [-1] * 7 and c[2, 0].tolist() == [-50, 0, 0.5]
    # the cap with a tie: four landmarks at 3 m, two places - the lower ids stay
    c, l = landmarks.virtual_scans(lm, poses[:1], node_num=3)
    assert l[0].tolist() == [0, 2, 9] and c[0].tolist() == [[1, 1, 0], [0, 3, 1], [3, 0, -1]]
    # keep: a mask over the landmarks
    keep = np.array([1, 1, 0, 0, 1, 1, 0, 1], bool)
    c, l = landmarks.virtual_scans(lm, poses[:1], node_num=4, keep=keep)
    assert l[0].tolist() == [2, 2, 5, -1] and c[0, :2].tolist() == [[0, -3, 2], [-3, 0, 3]]
    got = landmarks.virtual_scans(lm, poses, node_num=8)
    want = ref.virtual_scans(center, lm["label"], poses, node_num=8)
    assert (got[0].numpy() == want[0]).all() and (got[1].numpy() == want[1]).all()
    assert landmarks.virtual_scans(lm, np.zeros((0, 4)))[0].shape == (0, 100, 3)


def test_select_and_map_sharpness_on_known_numbers():
    from sg_pr_amd import landmarks, metrics
    lm = {"count": np.array([4, 1, 2, 1, 3], np.int32), "spread": np.array([0.5, 0.0, 1.0, 0.0, 0.0]),
          "sessions": np.array([0b011, 0b100, 0b100, 1 << 62, -1 << 63 | 1], np.int64)}
    m = metrics.map_sharpness(lm)
    assert m["landmarks"] == 3 and m["single"] == 0.4 and m["shared"] == 2 / 3
    assert m["sharpness"] == math.sqrt((4 * 0.25 + 2 * 1.0 + 3 * 0.0) / 9.0)
    m = metrics.map_sharpness(lm, min_count=1)
    assert m["landmarks"] == 5 and m["shared"] == 0.4
    assert math.isnan(metrics.map_sharpness(lm, min_count=9)["sharpness"])
    assert landmarks.select(lm).tolist() == [True] * 5
    assert landmarks.select(lm, min_count=2).tolist() == [True, False, True, False, True]
    assert landmarks.select(lm, min_sessions=2).tolist() == [True, False, False, False, True]
    assert landmarks.select(lm, min_count=4, min_sessions=2).tolist() == [True, False, False, False, False]


# ------------------------------------------------------------------ verification against the map
def pose_error(refined, truth):
    yaw = abs(math.atan2(refined[1] * truth[0] - refined[0] * truth[1], refined[0] * truth[0] + refined[1] * truth[1]))
    return math.hypot(refined[2] - truth[2], refined[3] - truth[3]), math.degrees(yaw)


def against_scan_and_map(w):
    """the last drive's scans (every 5th) verified against (a) their partner scan of the first drive and (b) the virtual
    scan at the partner's true pose, rendered from the landmark map of the first two drives at true poses
    -> medians (inliers a, inliers b, trans a, trans b, yaw a, yaw b)"""
    from sg_pr_amd import landmarks, synth
    lm = ref.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=[0, 100])
    keep = landmarks.select(lm, min_count=3)
    queries = np.arange(200, 300, 5)
    partner = queries - 200
    vc, vl = landmarks.virtual_scans(lm, w["truth"][partner], keep=keep)
    vc, vl = vc.numpy(), vl.numpy()
    rows = []
    for k, (q, p) in enumerate(zip(queries, partner)):
        truth = synth._se2_compose(synth._se2_inverse(w["truth"][p]), w["truth"][q])
        a = geo_ref.verify_pair(w["centers"][q], w["labels"][q], w["centers"][p], w["labels"][p], max_hyp=4096)
        b = geo_ref.verify_pair(w["centers"][q], w["labels"][q], vc[k], vl[k], max_hyp=4096)
        rows.append((a["inliers_refined"], b["inliers_refined"]) + tuple(
            v for pair in zip(pose_error(a["refined"], truth), pose_error(b["refined"], truth)) for v in pair))
    return np.median(np.array(rows, dtype=np.float64), axis=0)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_scan_verifies_better_against_the_map_than_against_a_scan(worlds, seed):
    ia, ib, ta, tb, ya, yb = against_scan_and_map(worlds[seed])
    print("seed %d: median refined inliers %.1f (scan) %.1f (map); translation error %.4f / %.4f m; yaw error %.4f / %.4f deg"
          % (seed, ia, ib, ta, tb, ya, yb))
    # (the translation error is smaller against the map on seeds 1..3 and larger by 0.001 m on seed 0, DESIGN.md §27: the
    # inliers are what holds on every seed, by 4.5 to 6)
    assert ib >= ia
