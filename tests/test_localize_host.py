"""Scan localisation (sgpr_localize_scans, include/sgpr_localize.h) without a GPU: the C-ABI surface of
the third header and its argument checks, the NumPy definition (tests/localize_ref.py) on synth.localize_world - the
conditions that make the stage worth having - its rules on hand-made cases, and mutants of the definition that must each
change an output."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localize_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
MIN_COS = math.cos(0.1)


@pytest.fixture(scope="module")
def worlds():
    from sg_pr_amd import synth
    return [synth.localize_world(seed) for seed in range(4)]


def run(w, L, **kw):
    return ref.localize(w["map"], w["cols"], w["T"], odo=w["odom"] if L > 1 else None, L=L, max_trans=1.0,
                        min_cos=MIN_COS, **kw)


def within(pose, truth):
    return np.hypot(pose[:, 2] - truth[:, 2], pose[:, 3] - truth[:, 3]) <= 1.0


def se2(yaw, x, y):
    return np.array([math.cos(yaw), math.sin(yaw), x, y])


IDENT = se2(0.0, 0.0, 0.0)


def at_places(places, **kw):
    """one query whose K candidates are map scans standing at `places` [(yaw, x, y)], seen through the identity"""
    m = np.array([se2(*p) for p in places])
    k = len(places)
    return ref.localize(m, np.arange(k)[None, :], np.tile(IDENT, (1, k, 1)), **kw)


# ------------------------------------------------------------------ C-ABI surface
def test_third_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, localize, posegraph
    text = open(os.path.join(REPO, "include", "sgpr_localize.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_localize_scans"] == localize.ABI_SYMBOLS
    assert abi.constants == {"SGPR_LOCALIZE_MAX_K": 64, "SGPR_LOCALIZE_MAX_LEN": 16, "SGPR_LOCALIZE_NO_HYPOTHESIS": 1,
                             "SGPR_LOCALIZE_DEGENERATE": 2}
    assert (localize.MAX_K, localize.MAX_LEN) == (64, 16) == (ref.MAX_K, ref.MAX_LEN)
    assert (localize.NO_HYPOTHESIS, localize.DEGENERATE) == (1, 2) == (ref.NO_HYPOTHESIS, ref.DEGENERATE)
    lib = localize.load_library()
    assert lib is engine.load_library()
    (name, restype, argtypes), = abi.functions
    fn = getattr(lib, name)
    assert fn.restype is restype is ctypes.c_int and list(fn.argtypes) == argtypes and len(argtypes) == 17
    assert argtypes[11] is argtypes[12] is ctypes.c_double and argtypes[0] is argtypes[16] is ctypes.c_void_p
    assert [argtypes[i] for i in (1, 5, 6, 9, 10)] == [ctypes.c_int] * 5
    # the build lists, and the other two headers are what they were
    assert "sgpr_localize.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_localize.h")) for h in _build.HEADERS[1:-1])
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any(n.startswith("sgpr_localize") for n in engine.ABI_SYMBOLS)
    assert len(posegraph.ABI_SYMBOLS) == 2


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import localize
    lib = localize.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    nan = float("nan")
    table = np.array([0, 4, 4, 8], np.int32)

    def call(map_=g, M=20, cols=g, T=g, accept=g, Q=8, K=4, odo=g, starts=None, ns=0, L=2, mt=1.0, mc=0.9, pose=g,
             stat=g, spread=g):
        s = None if starts is None else starts.ctypes.data
        return lib.sgpr_localize_scans(map_, M, cols, T, accept, Q, K, odo, s, ns, L, mt, mc, pose, stat, spread, None)

    def says(word):
        return b"sgpr_localize_scans" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("map_", "cols", "T", "odo", "pose", "stat", "spread"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(map_=None, M=0) == INVALID and says("NULL")          # (an empty map still needs a pointer)
    assert call(Q=-1) == INVALID and says("Q ") and call(M=-1) == INVALID and says("M ")
    for k in (0, -1, 65, 1 << 30):
        assert call(K=k) == INVALID and says("K "), k
    for n in (0, -1, 17, 1 << 30):
        assert call(L=n) == INVALID and says("L "), n
    for bad in (-1e-9, -float("inf"), nan):
        assert call(mt=bad) == INVALID and says("max_trans"), bad
    assert call(mc=nan) == INVALID and says("min_cos")
    # the session table
    assert call(starts=table, ns=0) == INVALID and says("session table")
    assert call(starts=None, ns=2) == INVALID and says("NULL session table")
    assert call(starts=table, ns=65) == INVALID and says("number of sessions")
    assert call(starts=table, ns=-1) == INVALID and says("number of sessions")
    assert call(starts=np.array([1, 4], np.int32), ns=2) == INVALID and says("start at 0")
    assert call(starts=np.array([0, 5, 4], np.int32), ns=3) == INVALID and says("decreasing")
    assert call(starts=np.array([0, 9], np.int32), ns=2) == INVALID and says("past 8")
    # Q == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    assert call(Q=0) == 0 and call(Q=0, starts=np.array([0, 0], np.int32), ns=2) == 0
    assert call(Q=0, map_=None, cols=None, T=None, accept=None, odo=None, pose=None, stat=None, spread=None, M=0) == 0
    assert call(Q=0, K=0) == INVALID and call(Q=0, L=17) == INVALID and call(Q=0, mt=nan) == INVALID
    assert call(Q=0, starts=np.array([0, 1], np.int32), ns=2) == INVALID and says("past 0")


# ------------------------------------------------------------------ the conditions, on the reference alone
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_consensus_over_scans_separates_a_pose_from_a_guess(worlds, seed):
    w = worlds[seed]
    assert w["map"].shape == (600, 4) and w["truth"].shape == w["odom"].shape == (200, 4)
    assert w["cols"].shape == (200, 8) and w["T"].shape == (200, 8, 4)
    pose8, stat8, _ = run(w, 8)
    acc8 = stat8[:, 0] >= 5
    pose1, stat1, _ = run(w, 1)
    acc1 = stat1[:, 0] >= 3
    slot0 = ref.compose(w["map"][w["cols"][:, 0]], w["T"][:, 0])
    figures = (acc8.mean(), within(pose8, w["truth"])[acc8].mean(), acc1.mean(), within(pose1, w["truth"])[acc1].mean(),
               within(slot0, w["truth"]).mean())
    print("seed %d: L=8 support>=5 accepted %.3f within 1 m %.3f; L=1 support>=3 accepted %.3f within 1 m %.3f; "
          "slot 0 within 1 m %.3f" % ((seed,) + figures))
    assert figures[0] >= 0.97 and figures[1] >= 0.99
    assert figures[2] <= 0.85 and figures[3] <= 0.95
    assert figures[4] <= 0.5


# ------------------------------------------------------------------ the rules, on hand-made cases
def test_three_agreeing_beat_two():
    places = [(0.0, 10.0, 10.0), (0.0, 0.1, 0.0), (0.01, 10.2, 10.1), (0.02, 0.0, 0.2), (-0.01, -0.1, 0.1)]
    pose, stat, spread = at_places(places)
    assert stat.tolist() == [[3, 5, 1, 0]]
    # slots 1, 3, 4 of 8: level 4 pairs (0,4) (1,5) (2,6) (3,7); level 2 pairs (0,2) (1,3); level 1 pair (0,1)
    sx = ((0.0 + -0.1) + 0.0) + ((0.1 + 0.0) + (0.0 + 0.0))
    sy = ((0.0 + 0.1) + 0.0) + ((0.0 + 0.0) + (0.2 + 0.0))
    assert pose[0, 2] == sx / 3.0 and pose[0, 3] == sy / 3.0
    # (the direction of a sum of unit vectors is the mean angle up to third order in the angles, here 0.02^3)
    assert abs(math.atan2(pose[0, 1], pose[0, 0]) - 0.01 / 3.0) < 1e-5 and abs(math.hypot(*pose[0, :2]) - 1.0) < 1e-15
    want = math.sqrt(sum((x - pose[0, 2]) ** 2 + (y - pose[0, 3]) ** 2 for _, x, y in (places[1], places[3], places[4])) / 3)
    assert abs(spread[0] - want) < 1e-15
    # the same three against three: the first complete cluster in slot order wins
    pose, stat, _ = at_places(places + [(0.0, 10.1, 10.0)])
    assert stat.tolist() == [[3, 6, 0, 0]] and abs(pose[0, 2] - 10.1) < 1e-12


def test_equal_supports_resolve_to_the_lowest_slot():
    pose, stat, _ = at_places([(0.0, 5.0, 5.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.1), (0.0, 5.0, 5.1)])
    assert stat.tolist() == [[2, 4, 0, 0]] and pose[0, 2] == 5.0
    # a chain a - b - c (a and c too far apart): b has the most support, and its supporters are a and c
    pose, stat, _ = at_places([(0.0, 0.0, 0.0), (0.0, 0.8, 0.0), (0.0, 1.6, 0.0)])
    assert stat.tolist() == [[3, 3, 1, 0]]
    # singletons: slot 0
    _, stat, spread = at_places([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 3.0, 0.0)])
    assert stat.tolist() == [[1, 3, 0, 0]] and spread[0] == 0.0


def test_sessions_bound_the_window():
    from sg_pr_amd import synth
    w = synth.localize_world(5, map_scans=100, queries=6, k=3, true_frac=1.0, alias_frac=0.0)
    kw = dict(odo=w["odom"], L=3)
    _, one, _ = ref.localize(w["map"], w["cols"], w["T"], **kw)
    assert one[:, 1].tolist() == [3, 6, 9, 9, 9, 9]
    _, two, _ = ref.localize(w["map"], w["cols"], w["T"], starts=[0, 2], **kw)
    assert two[:, 1].tolist() == [3, 6, 3, 6, 9, 9] and two[2, 2] < 3
    # an empty session in the table changes nothing; a one-query session sees itself alone
    _, gap, _ = ref.localize(w["map"], w["cols"], w["T"], starts=[0, 2, 2, 5], **kw)
    assert gap[:, 1].tolist() == [3, 6, 3, 6, 9, 3]
    # a query at a session start is the L = 1 answer, bit for bit, whatever the odometry holds
    bad = w["odom"].copy()
    bad[2] = np.nan
    p1, s1, d1 = ref.localize(w["map"], w["cols"], w["T"], L=1)
    p3, s3, d3 = ref.localize(w["map"], w["cols"], w["T"], starts=[0, 2], odo=bad, L=3)
    assert p3[2].tobytes() == p1[2].tobytes() and (s3[2] == s1[2]).all() and d3[2] == d1[2]
    assert s3[:, 1].tolist() == [3, 6, 3, 3, 6, 9]        # ... and the slots that touch odo[2] from later queries die


def test_dead_slots_and_no_hypothesis():
    m = np.array([se2(0.0, 1.0, 2.0), se2(0.0, 1.0, 2.5)])
    T = np.tile(IDENT, (2, 4, 1))
    cols = np.array([[-1, 2, 0x7fffffff, -5], [0, 1, -1, 1]])
    pose, stat, spread = ref.localize(m, cols, T)
    assert stat.tolist() == [[0, 0, -1, ref.NO_HYPOTHESIS], [3, 3, 0, 0]]
    assert np.isnan(pose[0]).all() and np.isnan(spread[0]) and pose[1, 2] == 1.0
    _, stat, _ = ref.localize(m, cols, T, accept=np.array([[1, 1, 1, 1], [0, 7, 1, 0]]))
    assert stat.tolist() == [[0, 0, -1, 1], [1, 1, 1, 0]]
    T[1, 3, 2] = np.inf
    assert ref.localize(m, cols, T)[1][1].tolist() == [2, 2, 0, 0]
    assert ref.localize(np.zeros((0, 4)), cols, T)[1].tolist() == [[0, 0, -1, 1]] * 2


def test_opposite_headings_are_degenerate():
    pose, stat, _ = at_places([(0.0, 0.0, 0.0), (math.pi, 0.0, 0.0)], min_cos=-1.0)
    assert stat.tolist() == [[2, 2, 0, 0]]                                     # sin(pi) != 0: a norm of 1e-16 still divides
    m = np.array([[1.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 0.5, 0.0]])
    pose, stat, _ = ref.localize(m, np.array([[1, 0]]), np.tile(IDENT, (1, 2, 1)), min_cos=-1.0)
    assert stat.tolist() == [[2, 2, 0, ref.DEGENERATE]] and pose[0].tolist() == [-1.0, 0.0, 0.25, 0.0]


def test_the_odometry_frame_decides_nothing(worlds):
    w = worlds[0]
    base = run(w, 8)[1]
    for frame in (se2(2.3, 0.0, 0.0), se2(0.0, -300.0, 120.0)):
        moved = ref.compose(frame[None, :], w["odom"])
        got = ref.localize(w["map"], w["cols"], w["T"], odo=moved, L=8, min_cos=MIN_COS)[1]
        assert (got == base).all()


# ------------------------------------------------------------------ mutants of the definition
def test_mutants_change_the_output(worlds):
    w = worlds[0]

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

    base = run(w, 8)
    assert not same(run(w, 8, tree=False), base)                  # a sequential sum in place of the tree
    assert not same(run(w, 8, transport_left=True), base)         # the transport composed on the left
    assert same(run(w, 8, tree=True, transport_left=False, test_self=False, ties_high=False), base)
    # self-agreement tested instead of counted: a slot whose (c, s) is short of a unit vector fails its own test
    m = np.array([[0.99, 0.0, 0.0, 0.0]])
    kw = dict(min_cos=0.999)
    assert ref.localize(m, [[0]], IDENT[None, None, :], **kw)[1].tolist() == [[1, 1, 0, 0]]
    assert ref.localize(m, [[0]], IDENT[None, None, :], test_self=True, **kw)[1].tolist() == [[0, 1, 0, 0]]
    # ties to the highest slot
    two = [(0.0, 5.0, 5.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.1), (0.0, 5.0, 5.1)]
    assert at_places(two)[1][0, 2] == 0 and at_places(two, ties_high=True)[1][0, 2] == 3


def test_tree_sum_is_the_stated_tree():
    rng = np.random.default_rng(0)
    for n, P2 in ((1, 1), (2, 2), (3, 4), (15, 16), (64, 64), (65, 128), (1024, 1024)):
        v = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, size=n)
        a = np.concatenate((v, np.zeros(P2 - n)))
        while a.size > 1:
            a = a[:a.size // 2] + a[a.size // 2:]
        assert ref.tree_sum(v, P2) == a[0], n
    assert math.copysign(1.0, ref.tree_sum(np.array([-0.0]), 1)) == -1.0        # one slot: no addition is made


# ------------------------------------------------------------------ the world and the metric
def test_localize_world_is_seeded_and_follows_the_recipe():
    from sg_pr_amd import synth
    a, b = synth.localize_world(2), synth.localize_world(2)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert a["cols"].dtype == a["index"].dtype == np.int32 and not np.array_equal(a["T"], synth.localize_world(3)["T"])
    assert (np.diff(a["index"]) == 1).all() and 0 <= a["index"][0] and a["index"][-1] < 600
    assert 0.3 < a["planted"].mean() < 0.5 and not (a["planted"] & a["aliased"]).any()
    assert (np.abs(a["cols"] - a["index"][:, None])[a["planted"]] <= 2).all()
    per_query = a["aliased"].sum(1)
    assert set(per_query.tolist()) <= {0, 1, 2, 3, 4} and 0.1 < (per_query > 0).mean() < 0.4
    # the true candidates say where the query is; the aliased ones of a query agree on another place
    P = ref.compose(a["map"][a["cols"]], a["T"])
    d = np.hypot(P[..., 2] - a["truth"][:, None, 2], P[..., 3] - a["truth"][:, None, 3])
    assert d[a["planted"]].max() < 1.5 and np.median(d[a["aliased"]]) > 20.0
    i = int(np.flatnonzero(per_query == 4)[0])
    Pa = P[i][a["aliased"][i]]
    # (their columns are random, so the yaw noise of 0.01 rad turns about a scan up to the map's diagonal away)
    lever = float(np.hypot(*(a["map"][:, 2:].max(0) - a["map"][:, 2:].min(0))))
    assert np.hypot(Pa[:, 2] - Pa[0, 2], Pa[:, 3] - Pa[0, 3]).max() < 1.5 + 2 * 4 * 0.01 * lever
    # the odometry is the truth in another frame, drifting slowly
    rel_t = ref.compose(ref.inverse(a["truth"][:-1]), a["truth"][1:])
    rel_o = ref.compose(ref.inverse(a["odom"][:-1]), a["odom"][1:])
    assert np.abs(rel_t - rel_o)[:, 2:].max() < 0.2 and np.hypot(*(a["odom"][0, 2:] - a["truth"][0, 2:])) > 10.0
    small = synth.localize_world(1, map_scans=50, queries=50, k=3)
    assert small["index"].tolist() == list(range(50)) and small["T"].shape == (50, 3, 4)


def test_localization_errors_on_a_known_offset():
    from sg_pr_amd import metrics
    truth = np.array([se2(0.3, 1.0, 2.0), se2(-3.1, -5.0, 0.0), se2(1.0, 0.0, 0.0), se2(0.0, 9.0, 9.0)])
    pose = np.array([se2(0.3 + math.radians(2.0), 1.0 + 3.0, 2.0 - 4.0), se2(3.1, -5.0, 0.5), se2(1.0, 0.0, 0.0),
                     [np.nan] * 4])
    e = metrics.localization_errors(pose, truth)
    np.testing.assert_allclose(e["trans_m"][:3], [5.0, 0.5, 0.0], atol=1e-12)
    np.testing.assert_allclose(e["yaw_deg"][:3], [2.0, math.degrees(2 * math.pi - 6.2), 0.0], atol=1e-9)
    assert np.isnan(e["trans_m"][3]) and np.isnan(e["yaw_deg"][3])
    assert e["median_trans_m"] == 0.5 and abs(e["median_yaw_deg"] - 2.0) < 1e-9
    none = metrics.localization_errors(np.full((2, 4), np.nan), truth[:2])
    assert np.isnan(none["median_trans_m"]) and np.isnan(none["median_yaw_deg"])
