"""The visibility tallies of a landmark map (sgpr_landmark_persist, include/sgpr_landmark_persist.h) without
a GPU: the C-ABI surface of the eighth header and its argument checks, the NumPy definition
(tests/landmark_persist_ref.py) on hand-made cases at every boundary of its rules, its additivity over the scans, mutants
of the definition that must each change an output, and synth.landmark_world - the map of two drives, the third aligned
to it and folded in, then tallied on the updated map: the landmarks it retires are the objects that have left."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_persist_ref as ref  # noqa: E402
import landmark_ref as lref  # noqa: E402
import landmark_update_ref as uref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
IDENT = (1.0, 0.0, 0.0, 0.0)
F32 = np.float32


def lm_of(center, label, use=None):
    lm = {"center": np.array(center, np.float64).reshape(-1, 3), "label": np.array(label, np.int32)}
    if use is not None:
        lm["use"] = np.array(use, np.uint8)
    return lm


def scans(nodes, labels, assoc, lm, poses=None, **kw):
    """scans given as lists of nodes, labels and associations through the reference"""
    q = len(nodes)
    return ref.persist(np.array(nodes, F32).reshape(q, -1, 3), np.array(labels, np.int32).reshape(q, -1),
                       np.array([IDENT] * q if poses is None else poses, np.float64), np.array(assoc, np.int32).reshape(q, -1), lm, **kw)


# ------------------------------------------------------------------ C-ABI surface
def test_eighth_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, landmarks, localize, posegraph
    text = open(os.path.join(REPO, "include", "sgpr_landmark_persist.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_landmark_persist_workspace_bytes", "sgpr_landmark_persist"] \
        == landmarks.PERSIST_ABI_SYMBOLS
    assert abi.constants == {} and abi.errors == {}
    lib = landmarks.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    (_, r0, a0), (_, r1, a1) = abi.functions
    assert r0 is ctypes.c_size_t and a0 == [ctypes.c_int] * 3
    assert r1 is ctypes.c_int and len(a1) == 25
    ints, doubles = (2, 3, 9, 11, 14), (12, 13, 15)
    assert [a1[i] for i in ints] == [ctypes.c_int] * 5 and [a1[i] for i in doubles] == [ctypes.c_double] * 3
    assert a1[23] is ctypes.c_size_t
    assert all(a1[i] is ctypes.c_void_p for i in range(25) if i not in ints + doubles + (23,))
    # the build lists, and the other seven headers are what they were
    assert "sgpr_landmark_persist.hip" in _build.SOURCES and "sgpr_landmark_update.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_landmark_persist.h")) for h in _build.HEADERS[1:-1])
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any("persist" in n for n in engine.ABI_SYMBOLS)
    assert landmarks.ABI_SYMBOLS == ["sgpr_landmark_workspace_bytes", "sgpr_landmark_map"]
    assert landmarks.REFINE_ABI_SYMBOLS == ["sgpr_landmark_refine_workspace_bytes", "sgpr_landmark_refine"]
    assert landmarks.ALIGN_ABI_SYMBOLS == ["sgpr_landmark_align_workspace_bytes", "sgpr_landmark_align"]
    assert landmarks.UPDATE_ABI_SYMBOLS == ["sgpr_landmark_update_workspace_bytes", "sgpr_landmark_update"]
    assert len(posegraph.ABI_SYMBOLS) == 2 and localize.ABI_SYMBOLS == ["sgpr_localize_scans"]


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import landmarks
    lib = landmarks.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    big = 1 << 40
    radius = (ctypes.c_double * 12)(*([0.75] * 12))
    inf, nan = float("inf"), float("nan")

    def call(centers=g, labels=g, Q=8, N=10, poses=g, assoc=g, lmc=g, lml=g, use=g, L=20, rad=radius, n_labels=12, max_range=50.0,
             margin=2.0, min_expected=5, ratio=0.3, expected=g, seen=g, keep=g, stat=g, view=g, num=g, ws=g, wsb=big):
        return lib.sgpr_landmark_persist(centers, labels, Q, N, poses, assoc, lmc, lml, use, L, rad, n_labels, max_range, margin,
                                         min_expected, ratio, expected, seen, keep, stat, view, num, ws, wsb, None)

    def says(word):
        return b"sgpr_landmark_persist" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("centers", "labels", "poses", "assoc", "lmc", "lml", "expected", "seen", "keep", "stat", "view", "num", "ws"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(rad=None) == INVALID and says("h_radius")
    for name in ("Q", "N", "L", "min_expected"):
        assert call(**{name: -1}) == INVALID and says(name) and says("negative"), name
    # (the accepted neighbours are asked with Q == 0: a call that passes its checks with Q N > 0 would go to the device)
    assert call(Q=0, min_expected=0) == 0
    for nl in (0, -1, 65):
        assert call(n_labels=nl) == INVALID and says("n_labels"), nl
    for bad in (-0.5, nan):
        r = (ctypes.c_double * 12)(*([0.75] * 5 + [bad] + [0.75] * 6))
        assert call(rad=r) == INVALID and says("radius of label 5")
        assert call(max_range=bad) == INVALID and says("max_range")
        assert call(margin=bad) == INVALID and says("margin")
        assert call(ratio=bad) == INVALID and says("max_seen_ratio")
    assert call(margin=inf) == INVALID and says("margin") and call(max_range=-inf) == INVALID and says("max_range")
    assert call(ratio=np.nextafter(1.0, 2.0)) == INVALID and says("max_seen_ratio") and call(ratio=inf) == INVALID
    assert call(Q=0, max_range=inf, margin=0.0, ratio=1.0) == 0 and call(Q=0, max_range=0.0, ratio=0.0) == 0
    assert call(Q=0, rad=(ctypes.c_double * 12)(*([inf] * 12))) == 0
    # node indices that leave int32
    assert call(Q=1 << 16, N=1 << 15) == INVALID and says("int32") and call(Q=0x7fffffff, N=0x7fffffff) == INVALID and says("int32")
    assert call(Q=0x7fffffff, N=1, wsb=0) == INVALID and says("workspace")
    need = lib.sgpr_landmark_persist_workspace_bytes(8, 10, 20)
    assert need > 0 and call(wsb=need - 1) == INVALID and says("workspace") and call(wsb=0) == INVALID and says("workspace")
    # the map and its outputs may be NULL where there is no landmark, the mask always
    per_landmark = dict(lmc=None, lml=None, use=None, expected=None, seen=None, keep=None)
    assert call(L=0, wsb=0, **per_landmark) == INVALID and says("workspace")
    assert call(L=0, stat=None, **per_landmark) == INVALID and says("NULL")
    assert call(use=None, wsb=0) == INVALID and says("workspace")
    # Q == 0 or N == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    none = dict(centers=None, labels=None, poses=None, assoc=None, stat=None, view=None, num=None, ws=None, wsb=0, **per_landmark)
    assert call(Q=0) == 0 and call(N=0) == 0 and call(Q=0, **none) == 0 and call(N=0, **none) == 0
    assert call(Q=0, L=-1) == INVALID and call(N=0, margin=-1.0) == INVALID and call(Q=0, rad=None) == INVALID
    assert call(N=0, n_labels=0) == INVALID and call(Q=0, ratio=1.5) == INVALID and call(N=0, min_expected=-2) == INVALID


def test_workspace_formula():
    from sg_pr_amd import landmarks
    for Q, N, L in ((1, 1, 0), (1, 1, 1), (2, 64, 11), (3, 100, 40), (5, 256, 300), (7, 100, 512), (7, 100, 513), (7, 100, 1100),
                    (4541, 100, 60000), (0, 100, 5), (7, 0, 5), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1 << 15, 1 << 15, 1),
                    (1 << 16, 1 << 15, 1), (0x7fffffff, 1, 7)):
        assert landmarks.persist_workspace_bytes(Q, N, L) == ref.workspace_bytes(Q, N, L), (Q, N, L)
    # no landmark: the smallest table (1024 slots of 8 + 4 + 4 bytes) and the counters; 12 bytes a landmark; the table doubles
    assert ref.workspace_bytes(1, 1, 0) == 1024 * 16 + 256 == ref.workspace_bytes(9999, 3, 0)
    assert ref.workspace_bytes(3, 100, 64) - ref.workspace_bytes(3, 100, 0) == 64 * 12
    assert ref.workspace_bytes(7, 100, 513) - ref.workspace_bytes(7, 100, 512) == 1024 * 16 + 3 * 256
    assert ref.workspace_bytes(9, 9, 7) % 256 == 0


# ------------------------------------------------------------------ the rules, on hand-made cases
FAR = [(10.0, 0.0, 0.0)]                      # a node that gives the scan a range of 10 m
KW = dict(max_range=50.0, margin=2.0, min_expected=1, max_seen_ratio=0.5)


def test_view_edge_is_inside_and_the_next_double_is_not():
    # v = 10 - 2 = 8; landmarks at 8 exactly, at the next double, and off both axes (d2 = 23.04 + 40.96, rounded to 64)
    assert 4.8 * 4.8 + 6.4 * 6.4 == 64.0
    lm = lm_of([(8.0, 0.0, 0.0), (np.nextafter(8.0, 9.0), 0.0, 0.0), (0.0, -8.0, 5.0), (0.0, np.nextafter(-8.0, -9.0), 0.0), (4.8, -6.4, 0.0)], [0] * 5)
    out = scans([FAR], [[0]], [[-2]], lm, **KW)
    assert out["view"].tolist() == [8.0] and out["expected"].tolist() == [1, 0, 1, 0, 1] and out["seen"].tolist() == [0] * 5
    assert out["keep"].tolist() == [0, 1, 0, 1, 0] and out["scan_stat"].tolist() == [[3, 0, 1, 0]] and out["num"].tolist() == [3, 3, 5, 1]
    # the distance is taken from the pose's translation, the range in the sensor frame: a rotation and a shift move the view
    out = scans([FAR], [[0]], [[-2]], lm, poses=[(0.0, 1.0, 100.0, 0.0)], **KW)
    assert out["view"].tolist() == [8.0] and out["expected"].tolist() == [0] * 5
    lm2 = lm_of([(108.0, 0.0, 0.0), (np.nextafter(108.0, 109.0), 0.0, 0.0)], [0, 0])
    out = scans([FAR], [[0]], [[-2]], lm2, poses=[(0.0, 1.0, 100.0, 0.0)], **KW)
    assert out["expected"].tolist() == [1, 0]
    # the sensor range caps the view: max_range 6 -> v = 4; +inf leaves the scan's own range
    out = scans([FAR], [[0]], [[-2]], lm_of([(4.0, 0.0, 0.0), (np.nextafter(4.0, 5.0), 0.0, 0.0)], [0, 0]), **dict(KW, max_range=6.0))
    assert out["view"].tolist() == [4.0] and out["expected"].tolist() == [1, 0]
    out = scans([FAR], [[0]], [[-2]], lm, **dict(KW, max_range=float("inf")))
    assert out["view"].tolist() == [8.0] and out["expected"].tolist() == [1, 0, 1, 0, 1]
    # the farthest LIVE node decides: a dead node farther out does not
    out = scans([FAR + [(30.0, 0.0, 0.0)]], [[0, -1]], [[-2, -2]], lm, **KW)
    assert out["view"].tolist() == [8.0] and out["scan_stat"].tolist() == [[3, 0, 1, 0]]


def test_margin_at_or_beyond_the_range_expects_nothing():
    lm = lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0])
    for margin, view in ((10.0, 0.0), (12.0, -2.0)):
        out = scans([FAR], [[0]], [[-2]], lm, **dict(KW, margin=margin))
        assert out["view"].tolist() == [view] and out["expected"].tolist() == [0, 0] and out["keep"].tolist() == [1, 1]
        assert out["num"].tolist() == [0, 0, 2, 0] and out["scan_stat"].tolist() == [[0, 0, 1, 0]]
    out = scans([FAR], [[0]], [[-2]], lm, **dict(KW, margin=np.nextafter(10.0, 0.0)))
    assert 0 < out["view"][0] < 1e-14 and out["expected"].tolist() == [1, 0] and out["num"].tolist() == [1, 1, 2, 1]   # a view of 2e-15 m holds the landmark under the sensor
    out = scans([FAR], [[0]], [[-2]], lm_of([(0.0, 0.0, 0.0)], [0]), **dict(KW, max_range=0.0, margin=0.0))
    assert out["view"].tolist() == [0.0] and out["expected"].tolist() == [0]


def test_a_scan_without_live_nodes_and_a_pose_that_is_not_finite():
    lm = lm_of([(1.0, 0.0, 0.0)], [0])
    out = scans([FAR, FAR, FAR], [[-1], [0], [0]], [[0], [0], [0]], lm, poses=[IDENT, (1.0, 0.0, np.nan, 0.0), (np.inf, 0.0, 0.0, 0.0)], **KW)
    assert out["view"].tolist() == [-2.0] * 3 and out["expected"].tolist() == [0] and out["seen"].tolist() == [0]
    assert out["scan_stat"].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1]] and out["num"].tolist() == [0, 0, 1, 0]
    # a node whose map point passes 2^37 is dead too
    out = scans([FAR], [[0]], [[0]], lm, poses=[(1.0, 0.0, 2.0 ** 37, 0.0)], **KW)
    assert out["scan_stat"].tolist() == [[0, 0, 0, 0]] and out["view"].tolist() == [-2.0]


def test_scans_are_counted_not_nodes():
    lm = lm_of([(1.0, 0.0, 0.0), (3.0, 0.0, 0.0)], [0, 0])
    nodes = [(1.0, 0.1, 0.0), (10.0, 0.0, 0.0), (1.1, 0.0, 0.0), (0.9, 0.0, 0.0)]
    out = scans([nodes, nodes], [[0] * 4] * 2, [[0, -2, 0, 0], [-2, -2, 0, 0]], lm, **KW)
    assert out["seen"].tolist() == [2, 0] and out["expected"].tolist() == [2, 2] and out["keep"].tolist() == [1, 0]
    assert out["scan_stat"].tolist() == [[2, 1, 4, 0]] * 2 and out["num"].tolist() == [1, 2, 2, 2]


def test_observed_beyond_the_view_counts_in_both_tallies():
    lm = lm_of([(20.0, 0.0, 0.0), (1.0, 0.0, 0.0)], [0, 0])
    out = scans([FAR + [(1.0, 0.0, 0.0)]], [[0, 0]], [[0, 1]], lm, **KW)          # v = 8: landmark 0 lies 20 m off
    assert out["expected"].tolist() == [1, 1] and out["seen"].tolist() == [1, 1] and out["scan_stat"].tolist() == [[2, 2, 2, 0]]
    # and with no view at all
    out = scans([FAR], [[0]], [[0]], lm, **dict(KW, margin=11.0))
    assert out["expected"].tolist() == [1, 0] and out["seen"].tolist() == [1, 0] and out["num"].tolist() == [0, 1, 2, 0]


def test_associations_that_do_not_observe():
    lm = lm_of([(1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (3.0, 0.0, 0.0), (4.0, 0.0, 0.0), (5.0, 0.0, 0.0), (np.nan, 0.0, 0.0)],
               [0, 1, 0, 3, -1, 0], use=[1, 1, 0, 1, 1, 1])
    radius = [0.75, 0.75, 0.75, 0.0]
    near = (1.0, 0.0, 0.0)
    # a wrong label; a masked landmark; a label of radius 0; a label outside the table; a centre that is not finite; values
    # outside the map; a dead node
    out = scans([FAR + [near] * 11], [[0] * 11 + [-1]], [[-2, 1, 2, 3, 4, 5, -3, 6, 2 ** 31 - 1, -1, -2 ** 31, 0]], lm, radius=radius, **KW)
    assert out["seen"].tolist() == [0] * 6 and out["expected"].tolist() == [1, 1, 0, 0, 0, 0]
    assert out["keep"].tolist() == [0, 0, 1, 1, 1, 1] and out["num"].tolist() == [2, 2, 2, 1] and out["scan_stat"].tolist() == [[2, 0, 11, 0]]
    out = scans([FAR + [near, near]], [[0, 0, 1]], [[-2, 0, 1]], lm, radius=radius, **KW)
    assert out["seen"].tolist() == [1, 1, 0, 0, 0, 0] and out["keep"].tolist() == [1] * 6


def test_decision_boundaries():
    lm = lm_of([(1.0, 0.0, 0.0)], [0])
    see, miss = FAR + [(1.0, 0.0, 0.0)], FAR + [(5.0, 5.0, 0.0)]

    def run(seen, missed, **kw):
        return scans([see] * seen + [miss] * missed, [[0, 0]] * (seen + missed), [[-2, 0]] * seen + [[-2, -2]] * missed, lm, **dict(KW, **kw))
    # expected == min_expected - 1 keeps, min_expected retires
    out = run(0, 4, min_expected=5)
    assert out["expected"].tolist() == [4] and out["keep"].tolist() == [1] and out["num"].tolist() == [0, 0, 1, 4]
    out = run(0, 5, min_expected=5)
    assert out["expected"].tolist() == [5] and out["keep"].tolist() == [0] and out["num"].tolist() == [1, 1, 1, 5]
    # seen == ratio * expected keeps; one fewer retires
    out = run(2, 2, max_seen_ratio=0.5)
    assert (out["seen"].tolist(), out["expected"].tolist(), out["keep"].tolist()) == ([2], [4], [1])
    out = run(1, 3, max_seen_ratio=0.5)
    assert (out["seen"].tolist(), out["expected"].tolist(), out["keep"].tolist()) == ([1], [4], [0])
    out = run(3, 7, max_seen_ratio=0.3)                          # the product is rounded: 0.3 * 10 is 3.0, equality
    assert 0.3 * 10.0 == 3.0 and out["keep"].tolist() == [1] and run(3, 8, max_seen_ratio=0.3)["keep"].tolist() == [0]
    assert run(0, 6, max_seen_ratio=0.0)["keep"].tolist() == [1] and run(6, 0, max_seen_ratio=1.0)["keep"].tolist() == [1]
    assert run(5, 1, max_seen_ratio=1.0)["keep"].tolist() == [0] and run(0, 1, min_expected=0, max_seen_ratio=1.0, margin=11.0)["keep"].tolist() == [1]     # 0 < 1.0 * 0 is false
    # a masked landmark is never retired, whatever was tallied around it
    out = scans([miss] * 6, [[0, 0]] * 6, [[-2, 0]] * 6, lm_of([(1.0, 0.0, 0.0)], [0], use=[0]), **KW)
    assert out["expected"].tolist() == [0] and out["seen"].tolist() == [0] and out["keep"].tolist() == [1] and out["num"].tolist() == [0, 0, 0, 6]


def test_no_landmark_and_no_scan():
    c, l, p, a, lm = ref.make_case(4, 30, 0, 3)
    out = ref.persist(c, l, p, a, lm, max_range=8.0, margin=0.5)
    assert out["expected"].size == out["seen"].size == out["keep"].size == 0 and out["num"][:3].tolist() == [0, 0, 0]
    assert out["scan_stat"].shape == (4, 4) and (out["scan_stat"][:, :2] == 0).all() and out["scan_stat"][0, 2] == 0
    c, l, p, a, lm = ref.make_case(4, 30, 50, 3)
    out = ref.persist(c[:0], l[:0], p[:0], a[:0], lm)
    assert out["expected"].tolist() == [0] * 50 and out["keep"].tolist() == [1] * 50 and out["view"].size == 0


# ------------------------------------------------------------------ additivity, mutants
def test_tallies_add_over_any_split_of_the_scans():
    c, l, p, a, lm = ref.make_case(40, 60, 300, 12)
    kw = dict(max_range=14.0, margin=1.0, min_expected=3)
    whole = ref.persist(c, l, p, a, lm, **kw)
    assert whole["seen"].sum() > 300 and (whole["expected"] > whole["seen"]).sum() > 50 and whole["num"][0] > 10
    rng = np.random.default_rng(5)
    for parts in ([slice(0, 17), slice(17, 40)], [slice(0, 1), slice(1, 2), slice(2, 40)], None):
        idx = [np.arange(40)[s] for s in parts] if parts else np.array_split(rng.permutation(40), 5)
        outs = [ref.persist(c[i], l[i], p[i], a[i], lm, **kw) for i in idx]
        assert sum(o["expected"].astype(np.int64) for o in outs).tolist() == whole["expected"].tolist()
        assert sum(o["seen"].astype(np.int64) for o in outs).tolist() == whole["seen"].tolist()
        assert sum(int(o["num"][3]) for o in outs) == whole["num"][3]
        order = np.concatenate(idx)
        assert np.concatenate([o["scan_stat"] for o in outs]).tobytes() == whole["scan_stat"][order].tobytes()
        assert np.concatenate([o["view"] for o in outs]).tobytes() == whole["view"][order].tobytes()
    assert (whole["seen"] <= whole["expected"]).all()


def test_mutants_change_an_output():
    assert set(ref.MUTANTS) >= {"count_nodes", "view_map_frame", "no_margin", "view_strict", "decide_le", "beyond_view_dropped",
                                "label_unchecked", "use_ignored"}
    c, l, p, a, lm = ref.make_case(12, 70, 200, 2)
    kw = dict(max_range=20.0, margin=1.0, min_expected=2, max_seen_ratio=0.5)
    base = ref.persist(c, l, p, a, lm, **kw)
    assert base["seen"].sum() > 150 and base["num"][0] > 5 and base["num"][3] >= 10
    changed = {}
    for m in ref.MUTANTS:
        out = ref.persist(c, l, p, a, lm, mutant=m, **kw)
        changed[m] = sorted(k for k in base if out[k].tobytes() != base[k].tobytes())
    # the two strictness mutants show at an exact boundary: the hand-made edge cases
    edge = lm_of([(8.0, 0.0, 0.0)], [0])
    assert scans([FAR], [[0]], [[-2]], edge, **KW)["expected"].tolist() == [1]
    assert scans([FAR], [[0]], [[-2]], edge, mutant="view_strict", **KW)["expected"].tolist() == [0]
    changed["view_strict"] = changed["view_strict"] or ["expected"]
    assert all(changed.values()), changed
    assert "seen" in changed["count_nodes"] and changed["view_map_frame"][-1] == "view" and "view" in changed["no_margin"]
    assert "keep" in changed["decide_le"] and changed["decide_le"][0] == "keep"
    assert "expected" in changed["beyond_view_dropped"] and "seen" not in changed["beyond_view_dropped"]
    assert "seen" in changed["label_unchecked"] and "seen" in changed["use_ignored"]
    again = ref.persist(c, l, p, a, lm, **kw)
    assert all(again[k].tobytes() == base[k].tobytes() for k in base)
    with pytest.raises(ValueError):
        ref.persist(c, l, p, a, lm, mutant="nope")


# ------------------------------------------------------------------ the planted world
def planted(seed):
    """DESIGN.md §33's procedure on synth.landmark_world(seed): the map of drives 0 and 1 at the true poses, drive 2
    displaced, aligned (gates 2.0 then 0.75 m on count >= 3), associated at iters = 0 and folded in, then tallied on the
    updated map with the update's node_landmark.  -> (world, map before, updated map, persist's outputs, stale bool [L]: the
    landmarks whose true object - the majority node_id of their nodes - existed during drive 0 or 1 only)"""
    from sg_pr_amd import synth
    w = synth.landmark_world(seed)
    N = w["labels"].shape[1]
    lm = lref.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=w["starts"][:2], radius=0.75, tau_z=0.75)
    rng = np.random.default_rng(500 + seed)
    X = synth._se2_compose(w["truth"][200:], synth._se2(rng.normal(0, 0.02, 100), rng.normal(0, 0.3, 100), rng.normal(0, 0.3, 100)))
    cen, lab = w["centers"][200:], w["labels"][200:]
    use = (lm["count"] >= 3).astype(np.uint8)
    for r in (2.0, 0.75):
        X = aref.align(cen, lab, X, lm["center"], lm["label"], lm_use=use, radius=r, iters=10, min_nodes=6)["poses"]
    assoc = aref.align(cen, lab, X, lm["center"], lm["label"], radius=0.75, tau_z=0.75, iters=0)["node_landmark"]
    up = uref.update(cen, lab, X, assoc, lm, session_base=2, node_base=200 * N)
    out = ref.persist(cen, lab, X, up["node_landmark"], up, max_range=50.0, margin=2.0, min_expected=5, max_seen_ratio=0.3)
    L = up["count"].size
    node = np.concatenate((lm["node_landmark"].reshape(-1), up["node_landmark"].reshape(-1)))
    obj = w["node_id"].reshape(-1)
    ok = (node >= 0) & (obj >= 0)
    votes = np.zeros((L, w["transient_session"].size), np.int64)
    np.add.at(votes, (node[ok], obj[ok]), 1)
    major = w["transient_session"][votes.argmax(1)]
    stale = (votes.sum(1) > 0) & ((major == 0) | (major == 1))
    return w, lm, up, out, stale


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_retired_landmarks_are_the_objects_that_left(seed):
    """Measured with this reference (seed 0..3): landmarks in use after the update 114, 112, 115, 99; stale among them 11,
    10, 16, 13; retired 10, 9, 15, 12, none of them not stale; the one stale landmark kept had expected 0, 1, 4, 2; lowest
    seen / expected of a judged landmark in use that is not stale 0.793, 0.750, 0.625, 0.800; highest of a stale one 0.0."""
    w, lm, up, out, stale = planted(seed)
    L0, L = lm["count"].size, up["count"].size
    in_use = up["count"] >= 3
    keep = out["keep"] != 0
    e, s = out["expected"].astype(np.float64), out["seen"].astype(np.float64)
    judged = out["expected"] >= 5
    with np.errstate(all="ignore"):
        ratio = s / e
    before = (stale & in_use).sum() / in_use.sum()
    after = (stale & in_use & keep).sum() / (in_use & keep).sum()
    low = ratio[in_use & ~stale & judged].min()
    new = (np.arange(L) >= L0) & judged
    stat = out["scan_stat"]
    print("seed %d: landmarks %d, in use %d, stale in use %d, retired %d, retired not stale %d, stale kept %d (expected %s), stale share "
          "%.3f -> %.3f, lowest ratio not stale %.3f, highest stale %.3f, new landmarks min %.2f median %.2f, per-scan median %.2f"
          % (seed, L, in_use.sum(), (stale & in_use).sum(), (~keep).sum(), (~keep & ~stale).sum(), (stale & in_use & keep).sum(),
             out["expected"][stale & in_use & keep].tolist(), before, after, low, ratio[stale & judged].max(), ratio[new].min(),
             np.median(ratio[new]), np.median(stat[:, 1] / np.maximum(stat[:, 0], 1))))
    assert not (~keep & ~stale).any()                            # no landmark that is not stale is retired
    assert not (stale & judged & keep).any() and (stale & judged).sum() >= 5      # every stale one that could be judged is
    assert before >= 0.08 and after <= 0.02
    assert low >= 0.5
    assert (out["seen"] <= out["expected"]).all()
    assert out["num"].tolist() == [(~keep).sum(), judged.sum(), L, 100] and (out["scan_stat"][:, 3] == 0).all()
