"""Pairwise-consistent loop closures (sgpr_closure_consistency / sgpr_consistent_set) without a GPU: the
C-ABI surface and its argument checks, the planar odometry convention, the NumPy definition (tests/consistency_ref.py)
on the planted world - the precondition tests/test_gpu_consistency.py leans on - and the greedy rule on hand-made
graphs."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consistency_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -7


# ------------------------------------------------------------------ C-ABI surface
def test_symbols_declared_exported_and_abi_version_kept():
    from sg_pr_amd import _build, engine
    header = open(os.path.join(REPO, "include", "sgpr.h")).read()
    lib = engine.load_library()
    for name in ("sgpr_closure_consistency", "sgpr_consistent_set"):
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert re.search(r"\bsize_t %s_workspace_bytes\s*\(" % name, header)
        assert name in engine.ABI_SYMBOLS and name + "_workspace_bytes" in engine.ABI_SYMBOLS
        assert getattr(lib, name) is not None and getattr(lib, name + "_workspace_bytes") is not None
    assert "sgpr_consistency.hip" in _build.SOURCES
    assert lib.sgpr_abi_version() == 11 == _build.header_abi_version()
    for name, value in (("MAX_CLOSURES", 16384), ("MAX_GROUPS", 4096)):
        assert int(re.search(r"#define SGPR_CONSISTENCY_%s (\d+)" % name, header).group(1)) == value
        assert getattr(engine, "CONSISTENCY_" + name) == value == getattr(ref, name)


def test_workspace_formulas():
    from sg_pr_amd import engine
    lib = engine.load_library()
    for c in (1, 2, 63, 64, 65, 129, 400, 4096, 16383, 16384):
        members = (4 * c + 255) // 256 * 256
        assert lib.sgpr_closure_consistency_workspace_bytes(c) == members + 96 * c, c
        assert lib.sgpr_consistent_set_workspace_bytes(c) == members, c
    for c in (0, -1, 16385, 1 << 30):          # nothing to do, or an invalid count: 0
        assert lib.sgpr_closure_consistency_workspace_bytes(c) == 0, c
        assert lib.sgpr_consistent_set_workspace_bytes(c) == 0, c


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with NULL or garbage device pointers: had the device been touched,
    the call would have failed with SGPR_E_HIP (no GPU) or crashed (a wild pointer)."""
    from sg_pr_amd import engine
    lib = engine.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    nan = float("nan")
    big = 1 << 30

    def cc(rows=g, cols=g, T=g, C=8, Xr=g, MR=5, Xc=g, MC=5, group=g, ng=1, mt=1.0, mc=0.99, lg=0.04, adj=g, deg=g, ws=g,
           wb=big):
        return lib.sgpr_closure_consistency(rows, cols, T, C, Xr, MR, Xc, MC, group, ng, mt, mc, lg, adj, deg, ws, wb, None)

    def cs(adj=g, C=8, group=g, ng=1, rank=g, size=g, ws=g, wb=big):
        return lib.sgpr_consistent_set(adj, C, group, ng, rank, size, ws, wb, None)

    def says(word):
        return word.encode() in lib.sgpr_last_error()

    for name in ("rows", "cols", "T", "Xr", "Xc", "group", "adj", "deg"):
        assert cc(**{name: None}) == INVALID, name
        assert says("sgpr_closure_consistency") and says("NULL")
    for name in ("adj", "group", "rank", "size"):
        assert cs(**{name: None}) == INVALID, name
        assert says("sgpr_consistent_set") and says("NULL")
    for call in (cc, cs):
        for c in (-1, 16385, 1 << 30):
            assert call(C=c) == INVALID and says("C "), c
        for ng in (0, -1, 4097):
            assert call(ng=ng) == INVALID and says("n_groups"), ng
        assert call(ws=None) == WORKSPACE and says("workspace")
    assert cc(MR=-1) == INVALID and says("pose table")
    assert cc(MC=-1) == INVALID and says("pose table")
    for name in ("mt", "lg"):
        assert cc(**{name: -0.5}) == INVALID and says("max_trans"), name
        assert cc(**{name: nan}) == INVALID and says("max_trans"), name
    assert cc(mc=nan) == INVALID and says("min_cos")
    assert cc(wb=lib.sgpr_closure_consistency_workspace_bytes(8) - 1) == WORKSPACE
    assert cs(wb=lib.sgpr_consistent_set_workspace_bytes(8) - 1) == WORKSPACE
    # C == 0 succeeds without a launch, whatever the pointers are
    assert cc(C=0) == 0
    assert cc(C=0, rows=None, cols=None, T=None, Xr=None, Xc=None, group=None, adj=None, deg=None, ws=None, wb=0) == 0
    assert cs(C=0, adj=None, group=None, rank=None, size=None, ws=None, wb=0) == 0
    # ... but not with a bad count beside it
    assert cc(C=0, ng=0) == INVALID and cs(C=0, ng=4097) == INVALID and cc(C=0, mt=nan) == INVALID


# ------------------------------------------------------------------ conventions
def test_planar_odometry_agrees_with_closure_pose_errors():
    """the closure inverse(X[col]) o X[row] of the planar poses is the truth closure_pose_errors measures against"""
    from sg_pr_amd import metrics, synth
    poses = synth.world_sequence(num_graphs=90, node_num=60, seed=3)[3]
    X = metrics.planar_odometry(poses)
    assert X.dtype == np.float64 and X.shape == (90, 4)
    np.testing.assert_array_equal(X[:, 2], poses[:, 3])
    np.testing.assert_array_equal(X[:, 3], poses[:, 11])
    np.testing.assert_allclose(np.arctan2(X[:, 1], X[:, 0]), np.arctan2(poses[:, 2], poses[:, 0]), atol=1e-15)
    rng = np.random.default_rng(0)
    rows, cols = rng.integers(0, 90, size=200), rng.integers(0, 90, size=200)
    T = ref.compose(ref.inverse(X[cols]), X[rows])
    err = metrics.closure_pose_errors({"refined": T, "flags": np.zeros(200, np.int32)}, rows, cols, poses)
    assert err["yaw_deg"].max() < 1e-9 and err["trans_m"].max() < 1e-9
    # such closures are consistent with one another to rounding: one complete group
    adj, degree, members = ref.closure_consistency(rows, cols, T, X, X, np.zeros(200, np.int32), 1, 1e-6, math.cos(1e-6), 0.0)
    assert (degree == 199).all() and (members == 0).all()


def test_se2_algebra_of_the_reference():
    rng = np.random.default_rng(1)
    yaw = rng.uniform(-3, 3, size=(3, 50))
    A, B, Cc = (np.stack((np.cos(y), np.sin(y), rng.normal(size=50) * 30, rng.normal(size=50) * 30), axis=1) for y in yaw)
    eye = np.array([1.0, 0.0, 0.0, 0.0])
    np.testing.assert_allclose(ref.compose(A, ref.inverse(A)), np.broadcast_to(eye, (50, 4)), atol=1e-12)
    np.testing.assert_allclose(ref.compose(ref.compose(A, B), Cc), ref.compose(A, ref.compose(B, Cc)), atol=1e-10)
    p = rng.normal(size=(50, 2))
    act = lambda E, p: np.stack((E[:, 0] * p[:, 0] - E[:, 1] * p[:, 1] + E[:, 2], E[:, 1] * p[:, 0] + E[:, 0] * p[:, 1] + E[:, 3]), 1)  # noqa: E731
    np.testing.assert_allclose(act(ref.compose(A, B), p), act(A, act(B, p)), atol=1e-10)


# ------------------------------------------------------------------ the planted world: why a clique and not a threshold
@pytest.mark.parametrize("outlier_frac", [0.5, 0.8])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_selects_the_planted_inliers_and_no_aliased_closure(seed, outlier_frac):
    from sg_pr_amd import synth
    w = synth.closure_world(seed, outlier_frac=outlier_frac)
    C = w["rows"].size
    assert C == 400 and w["aliased"].sum() == 30 and not (w["aliased"] & w["planted"]).any()
    assert w["planted"].sum() == round(400 * (1 - outlier_frac))
    adj, degree, members = ref.closure_consistency(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], np.zeros(C, np.int32), 1,
                                                   1.0, math.cos(0.06), 0.04)
    assert (members == 0).all()
    mat = ref.unpack_bits(adj, C)
    assert (mat == mat.T).all() and not mat.diagonal().any() and (degree == mat.sum(1)).all()
    rank, size = ref.consistent_set(adj, members, 1)
    sel = rank >= 0
    assert size[0] == sel.sum() and sorted(rank[sel]) == list(range(size[0]))
    assert mat[np.ix_(sel, sel)].sum() == size[0] * (size[0] - 1)            # a clique
    assert not (sel & ~w["planted"]).any()                                   # no outlier ...
    assert not (sel & w["aliased"]).any()                                    # ... none of the aliased cluster
    assert (sel & w["planted"]).sum() >= 0.95 * w["planted"].sum()
    # a support threshold accepts the aliased cluster: the gap the clique closes
    assert ((degree >= 10) & w["aliased"]).sum() >= 25
    # the counting reference is the stated rule
    lit_rank, lit_size = ref.consistent_set_literal(adj, members, 1)
    assert (lit_rank == rank).all() and (lit_size == size).all()


# ------------------------------------------------------------------ the greedy rule on hand-made graphs
def _matrix(C, edges, both=True):
    mat = np.zeros((C, C), dtype=bool)
    for a, b in edges:
        mat[a, b] = True
        if both:
            mat[b, a] = True
    return mat


def _clique(nodes):
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


@pytest.mark.parametrize("solver", [ref.consistent_set, ref.consistent_set_literal])
def test_greedy_rule_on_hand_made_graphs(solver):
    # two disjoint cliques of 5 and 4 in one group: the 5
    five, four = [1, 3, 4, 6, 8], [0, 2, 5, 7]
    adj = ref.pack_bits(_matrix(10, _clique(five) + _clique(four)))
    rank, size = solver(adj, np.zeros(10, np.int32), 1)
    assert size.tolist() == [5] and rank[five].tolist() == [0, 1, 2, 3, 4] and (rank[four] == -1).all() and rank[9] == -1
    # ties go to the lowest index: two triangles, then within the chosen one ascending
    adj = ref.pack_bits(_matrix(6, _clique([3, 4, 5]) + _clique([0, 1, 2])))
    rank, size = solver(adj, np.zeros(6, np.int32), 1)
    assert rank.tolist() == [0, 1, 2, -1, -1, -1] and size.tolist() == [3]
    # no edges at all: a clique of one, the lowest index
    rank, size = solver(ref.pack_bits(np.zeros((4, 4), bool)), np.zeros(4, np.int32), 1)
    assert rank.tolist() == [0, -1, -1, -1] and size.tolist() == [1]
    # groups are separate problems; a closure of no group is never selected; an empty group has size 0
    group = np.array([0, 0, 0, 2, 2, -1, 7, 2], np.int32)
    adj = ref.pack_bits(_matrix(8, _clique([0, 1, 2]) + _clique([3, 4, 7]) + [(2, 3), (5, 0), (6, 1)]))
    rank, size = solver(adj, group, 3)
    assert rank.tolist() == [0, 1, 2, 0, 1, -1, -1, 2] and size.tolist() == [3, 0, 3]
    # diagonal bits and bits beyond C are ignored
    mat = _matrix(5, _clique([1, 2, 3]))
    clean = solver(ref.pack_bits(mat), np.zeros(5, np.int32), 1)
    junk = ref.pack_bits(mat | np.eye(5, dtype=bool)).view(np.uint64) | np.uint64(0xffffffffffffffe0)
    dirty = solver(junk.view(np.int64), np.zeros(5, np.int32), 1)
    assert clean[0].tolist() == dirty[0].tolist() == [-1, 0, 1, 2, -1] and clean[1].tolist() == dirty[1].tolist() == [3]
    # an asymmetric matrix still terminates: rows decide (0 -> 1 -> 2 -> 0 one way round)
    adj = ref.pack_bits(_matrix(3, [(0, 1), (1, 2), (2, 0)], both=False))
    rank, size = solver(adj, np.zeros(3, np.int32), 1)
    assert rank.tolist() == [0, 1, -1] and size.tolist() == [2]


def test_void_closures_of_the_reference():
    from sg_pr_amd import synth
    w = synth.closure_world(5, scans=60, closures=40, outlier_frac=0.25, alias=0)
    rows, cols, T, group = w["rows"].copy(), w["cols"].copy(), w["T"].copy(), np.zeros(40, np.int32)
    rows[3], cols[5], rows[7], cols[9], group[11], group[13] = -1, -1, 60, 60, -1, 1
    T[15, 0], T[17, 3] = np.nan, np.inf
    Xr, Xc = w["Xr"].copy(), w["Xc"].copy()
    Xr[rows[19], 2], Xc[cols[21], 1] = -np.inf, np.nan
    void = np.zeros(40, bool)
    void[[3, 5, 7, 9, 11, 13, 15, 17]] = True
    void |= (rows == rows[19]) | (cols == cols[21])
    adj, degree, members = ref.closure_consistency(rows, cols, T, Xr, Xc, group, 1, 1.0, math.cos(0.06), 0.04)
    mat = ref.unpack_bits(adj, 40)
    assert (members == np.where(void, -1, 0)).all()
    assert not mat[void].any() and not mat[:, void].any() and (degree[void] == 0).all()
    clean = ref.closure_consistency(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], np.zeros(40, np.int32), 1, 1.0,
                                    math.cos(0.06), 0.04)
    keep = ~void
    assert (mat[np.ix_(keep, keep)] == ref.unpack_bits(clean[0], 40)[np.ix_(keep, keep)]).all()      # neighbours unaffected
    rank, size = ref.consistent_set(adj, members, 1)
    assert (rank[void] == -1).all() and size[0] == (rank >= 0).sum() > 10


def test_closure_world_is_seeded_and_shaped():
    from sg_pr_amd import synth
    a, b = synth.closure_world(2, outlier_frac=0.5), synth.closure_world(2, outlier_frac=0.5)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert a["rows"].dtype == np.int32 and a["T"].shape == (400, 4) and a["Xr"].shape == a["Xc"].shape == (600, 4)
    assert not np.array_equal(a["T"], synth.closure_world(3, outlier_frac=0.5)["T"])
    # true closures pair scans within +-2 indices; the two drives live in unrelated frames
    assert np.abs(a["rows"][a["planted"]] - a["cols"][a["planted"]]).max() <= 2
    assert np.hypot(*(a["Xr"][:, 2:] - a["Xc"][:, 2:]).T).max() > 20
