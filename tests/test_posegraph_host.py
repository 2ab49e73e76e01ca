"""Planar pose-graph relaxation (sgpr_posegraph_optimize, include/sgpr_posegraph.h) without a GPU: the
C-ABI surface of the second header and its argument checks, the NumPy definition (tests/posegraph_ref.py) on
synth.drift_world - the condition tests/test_gpu_posegraph.py leans on - its agreement with a direct sparse solve, its
rules, and mutants of the definition that must each change the output."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegraph_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -7
# the largest |reference at rel_tol 1e-12 - direct solve| over drift_world seeds 0..3 measured 1.6e-10 (seed 0; DESIGN.md
# §25); ten times that, because the gap follows each seed's conditioning
DIRECT_GAP = 1.6e-9


@pytest.fixture(scope="module")
def worlds():
    from sg_pr_amd import synth
    return [synth.drift_world(seed) for seed in range(4)]


def run(w, **kw):
    return ref.optimize(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"], **kw)


# ------------------------------------------------------------------ C-ABI surface
def test_second_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, posegraph
    text = open(os.path.join(REPO, "include", "sgpr_posegraph.h")).read()
    abi = _build.parse_header(text)
    names = [n for n, _, _ in abi.functions]
    assert names == ["sgpr_posegraph_optimize_workspace_bytes", "sgpr_posegraph_optimize"] == posegraph.ABI_SYMBOLS
    assert abi.constants["SGPR_POSEGRAPH_MAX_SCANS"] == 65536 == posegraph.MAX_SCANS == ref.MAX_SCANS
    assert abi.constants["SGPR_POSEGRAPH_MAX_CLOSURES"] == 16384 == posegraph.MAX_CLOSURES == ref.MAX_CLOSURES
    assert abi.constants["SGPR_POSEGRAPH_MAX_ITERS"] == 65536 == posegraph.MAX_ITERS == ref.MAX_ITERS
    assert abi.constants["SGPR_POSEGRAPH_SEGMENT"] == 64 == posegraph.SEGMENT == ref.SEGMENT
    assert (posegraph.NONFINITE, posegraph.NO_ANCHOR, posegraph.DEGENERATE) == (ref.NONFINITE, ref.NO_ANCHOR, ref.DEGENERATE)
    assert (posegraph.CONVERGED, posegraph.STOP_MAX_ITERS, posegraph.BREAKDOWN) == (ref.CONVERGED, ref.STOP_MAX_ITERS, ref.BREAKDOWN)
    assert (posegraph.W_ODO, posegraph.W_CLO) == (ref.W_ODO, ref.W_CLO)
    lib = posegraph.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    fn = lib.sgpr_posegraph_optimize
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 22
    assert fn.argtypes[10:14] == [ctypes.c_double] * 4 and fn.argtypes[15] is ctypes.c_double
    assert fn.argtypes[20] is ctypes.c_size_t and fn.argtypes[0] is ctypes.c_void_p
    assert "sgpr_posegraph.hip" in _build.SOURCES and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h"))
    # the first header is what it was
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any(n.startswith("sgpr_posegraph") for n in engine.ABI_SYMBOLS)


def test_workspace_formula():
    from sg_pr_amd import posegraph
    lib = posegraph.load_library()
    for m, c in ((1, 0), (1, 1), (63, 5), (64, 0), (65, 65), (600, 120), (4500, 450), (65536, 16384)):
        assert lib.sgpr_posegraph_optimize_workspace_bytes(m, c) == 8192 + 192 * m + 64 * c + 2624 * (m // 64 + 64), (m, c)
    for m, c in ((0, 0), (0, 5), (-1, 0), (65537, 0), (10, -1), (10, 16385), (1 << 30, 1)):
        assert lib.sgpr_posegraph_optimize_workspace_bytes(m, c) == 0, (m, c)


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with garbage device pointers: had the device been touched, the call
    would have failed with SGPR_E_HIP (no GPU) or crashed (a wild pointer)."""
    from sg_pr_amd import posegraph
    lib = posegraph.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    nan, inf, big = float("nan"), float("inf"), 1 << 40
    table = np.array([0, 4, 4, 8], np.int32)

    def call(X=g, M=8, starts=None, ns=0, rows=g, cols=g, T=g, weight=None, C=5, fixed=None, wor=1.0, wot=1.0, wcr=1.0,
             wct=1.0, iters=10, tol=1e-9, out=g, info=g, resid=g, ws=g, wb=big):
        s = None if starts is None else starts.ctypes.data
        return lib.sgpr_posegraph_optimize(X, M, s, ns, rows, cols, T, weight, C, fixed, wor, wot, wcr, wct, iters, tol, out,
                                           info, resid, ws, wb, None)

    def says(word):
        return b"sgpr_posegraph_optimize" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("X", "rows", "cols", "T", "out", "info", "resid"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    for m in (-1, 65537, 1 << 30):
        assert call(M=m) == INVALID and says("M "), m
    for c in (-1, 16385, 1 << 30):
        assert call(C=c) == INVALID and says("C "), c
    for it in (-1, 65537):
        assert call(iters=it) == INVALID and says("max_iters"), it
    for name in ("wor", "wot", "wcr", "wct"):
        for bad in (0.0, -1.0, nan, inf):
            assert call(**{name: bad}) == INVALID and says("weight"), (name, bad)
    for bad in (-1e-9, nan):
        assert call(tol=bad) == INVALID and says("rel_tol"), bad
    # the session table
    assert call(starts=table, ns=0) == INVALID and says("session table")
    assert call(starts=None, ns=2) == INVALID and says("NULL session table")
    assert call(starts=table, ns=65) == INVALID and says("number of sessions")
    assert call(starts=table, ns=-1) == INVALID and says("number of sessions")
    assert call(starts=np.array([1, 4], np.int32), ns=2) == INVALID and says("start at 0")
    assert call(starts=np.array([0, 5, 4], np.int32), ns=3) == INVALID and says("decreasing")
    assert call(starts=np.array([0, 9], np.int32), ns=2) == INVALID and says("past 8")
    # the workspace
    need = lib.sgpr_posegraph_optimize_workspace_bytes(8, 5)
    assert call(ws=None) == WORKSPACE and says("workspace")
    assert call(wb=need - 1, starts=table, ns=4) == WORKSPACE and says(str(need))
    # M == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    assert call(M=0, starts=np.array([0, 0], np.int32), ns=2) == 0
    assert call(M=0, X=None, rows=None, cols=None, T=None, out=None, info=None, resid=None, ws=None, wb=0, C=0) == 0
    assert call(M=0, wor=nan) == INVALID and call(M=0, C=-1) == INVALID and call(M=0, tol=-1.0) == INVALID
    assert call(M=0, starts=np.array([0, 1], np.int32), ns=2) == INVALID and says("past 0")


# ------------------------------------------------------------------ the condition, on the reference alone
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_merges_the_map_and_spreads_the_drift(worlds, seed):
    from sg_pr_amd import metrics
    w = worlds[seed]
    assert w["odom"].shape == w["truth"].shape == (600, 4) and w["starts"].tolist() == [0, 300]
    out, info, resid = run(w)
    assert info[0] == 0 and info[3] == info[4] == ref.CONVERGED and info[5] == 120 and info[6] == 599 and info[7] == 2
    assert 0 < info[1] < 200 and 0 < info[2] < 200
    assert resid[1] <= 1e-18 * resid[0] and resid[3] <= 1e-18 * resid[2]
    before, after = metrics.trajectory_error(w["odom"], w["truth"]), metrics.trajectory_error(out, w["truth"])
    per_session = metrics.trajectory_error(w["odom"], w["truth"], w["starts"])
    print("seed %d: merged error %.2f m -> %.3f m, per-session odometry %s, iterations %d + %d"
          % (seed, before, after, per_session.round(3).tolist(), info[1], info[2]))
    assert after <= before / 20.0
    assert after <= 1.25 * np.sqrt(np.mean(per_session ** 2))
    np.testing.assert_array_equal(out[0], w["odom"][0])                     # the anchor
    np.testing.assert_allclose(np.hypot(out[:, 0], out[:, 1]), 1.0, atol=1e-15)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_agrees_with_a_direct_solve(worlds, seed):
    import scipy.sparse.linalg
    w = worlds[seed]
    out, info, _ = run(w, rel_tol=1e-12)
    direct = ref.normal_equations(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"])(scipy.sparse.linalg.spsolve)
    gap = np.abs(out - direct).max()
    print("seed %d: gap to the direct solve %.3g after %d + %d iterations" % (seed, gap, info[1], info[2]))
    assert info[3] == info[4] == ref.CONVERGED and gap <= DIRECT_GAP


def test_segment_preconditioner_earns_its_place(worlds):
    w = worlds[0]
    seg, jac = run(w)[1], run(w, precond="jacobi")[1]
    assert jac[3] == jac[4] == ref.CONVERGED
    assert 3 * seg[1] < jac[1] and 3 * seg[2] < jac[2]


# ------------------------------------------------------------------ the rules
def small(seed=7, scans=40, sessions=3, closures=30):
    from sg_pr_amd import synth
    return synth.drift_world(seed, scans=scans, sessions=sessions, closures=closures)


def test_an_inert_session_keeps_its_bits():
    w = small()
    keep = (w["rows"] < 80) & (w["cols"] < 80)                       # no closure reaches the third session
    out, info, _ = ref.optimize(w["odom"], w["rows"][keep], w["cols"][keep], w["T"][keep], starts=w["starts"])
    assert info[0] == 0 and info[7] == 2 and info[6] == 79 and info[5] == keep.sum()
    assert out[80:].tobytes() == w["odom"][80:].tobytes() and out[0].tobytes() == w["odom"][0].tobytes()
    assert (out[1:80] != w["odom"][1:80]).any(axis=1).all()
    # anchored in the third session instead: the first two are tied to each other but to no anchor
    fixed = np.zeros(120, bool)
    fixed[100] = True
    out, info, _ = ref.optimize(w["odom"], w["rows"][keep], w["cols"][keep], w["T"][keep], starts=w["starts"], fixed=fixed)
    assert info[7] == 1 and info[6] == 39 and out[:80].tobytes() == w["odom"][:80].tobytes()


def test_status_flags_return_the_input():
    w = small()
    out, info, resid = run(w, fixed=np.zeros(120, bool))
    assert info.tolist() == [ref.NO_ANCHOR, 0, 0, 0, 0, 0, 0, 0] and not resid.any()
    assert out.tobytes() == w["odom"].tobytes()
    for k, j, v in ((5, 2, np.nan), (119, 0, np.inf), (60, 3, -np.inf)):
        X = w["odom"].copy()
        X[k, j] = v
        out, info, resid = ref.optimize(X, w["rows"], w["cols"], w["T"], starts=w["starts"])
        assert info.tolist() == [ref.NONFINITE, 0, 0, 0, 0, 0, 0, 0] and out.tobytes() == X.tobytes()
    X = w["odom"].copy()
    X[17, :2] = 0.0
    out, info, _ = ref.optimize(X, w["rows"], w["cols"], w["T"], starts=w["starts"], fixed=np.zeros(120, bool))
    assert info[0] == ref.NONFINITE | ref.NO_ANCHOR and out.tobytes() == X.tobytes()


def test_stopping_rules():
    w = small()
    out, info, resid = run(w, max_iters=0)
    assert info[1:5].tolist() == [0, 0, ref.STOP_MAX_ITERS, ref.STOP_MAX_ITERS] and resid[0] == resid[1] > 0
    # (stage T still sees the normalised rotations of stage R's start: positions keep their bits)
    assert out[:, 2:].tobytes() == w["odom"][:, 2:].tobytes()
    full = run(w)[1]
    out, info, resid = run(w, max_iters=int(full[1]) - 1)
    assert info[1] == full[1] - 1 and info[3] == ref.STOP_MAX_ITERS
    # no closures: the input
    out, info, _ = ref.optimize(w["odom"], [], [], np.zeros((0, 4)), starts=w["starts"])
    assert out.tobytes() == w["odom"].tobytes() and info.tolist() == [0, 0, 0, 0, 0, 0, 39, 1]


def test_closures_that_agree_with_the_odometry_stop_at_once():
    """rz0 == 0: a grid-aligned drive whose closures are its own relative poses, every product exact"""
    M = 70
    X = np.zeros((M, 4))
    X[:, 0] = 1.0
    X[:, 2] = np.arange(M) * 2.0
    X[:, 3] = 3.0
    rows, cols = np.array([60, 5, 33]), np.array([2, 50, 30])
    T = np.stack((np.ones(3), np.zeros(3), X[rows, 2] - X[cols, 2], np.zeros(3)), axis=1)
    out, info, resid = ref.optimize(X, rows, cols, T)
    assert info.tolist() == [0, 0, 0, ref.CONVERGED, ref.CONVERGED, 3, M - 1, 1] and not resid.any()
    assert out.tobytes() == X.tobytes()


def test_void_closures_take_no_part():
    w = small()
    rows, cols, T = w["rows"].copy(), w["cols"].copy(), w["T"].copy()
    weight = np.ones(30)
    rows[1], cols[2], rows[3], cols[4] = -1, -1, 120, 120
    cols[5] = rows[5]
    T[6, 0], T[7, 3], T[8, :2] = np.nan, np.inf, 0.0
    weight[9], weight[10], weight[11], weight[12] = 0.0, -1.0, np.nan, np.inf
    live = np.ones(30, bool)
    live[1:13] = False
    got = ref.optimize(w["odom"], rows, cols, T, starts=w["starts"], weight=weight)
    want = ref.optimize(w["odom"], rows[live], cols[live], T[live], starts=w["starts"])
    assert got[1][5] == 18 and got[0].tobytes() == want[0].tobytes() and (got[1] == want[1]).all()


# ------------------------------------------------------------------ mutants of the definition
def test_mutants_change_the_output(worlds):
    w = worlds[0]
    base = run(w)[0]
    # Jacobi in place of the segment solve, and a segment of 63
    assert run(w, precond="jacobi")[0].tobytes() != base.tobytes()
    assert run(w, segment=63)[0].tobytes() != base.tobytes()
    # a sequential sum in place of the tree, tail terms before head terms
    assert run(w, tree=False)[0].tobytes() != base.tobytes()
    assert run(w, tail_first=True)[0].tobytes() != base.tobytes()
    # a fused product in the inner product (exact rational arithmetic: a small map)
    s = small()
    assert run(s, fused=True)[0].tobytes() != run(s)[0].tobytes()
    # ... while the switches at their defaults are the definition
    assert run(w, precond="segment", segment=64, tree=True, tail_first=False, fused=False)[0].tobytes() == base.tobytes()


def test_tree_sum_is_the_stated_tree():
    rng = np.random.default_rng(0)
    for n in (1, 2, 1023, 1024, 1025, 2049, 5000):
        v = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, size=n)
        a = np.zeros(((n + 1023) // 1024) * 1024)
        a[:n] = v

        def tree(x):
            while x.size > 1:
                x = x[:x.size // 2] + x[x.size // 2:]
            return x[0]
        sums = np.array([tree(c) for c in a.reshape(-1, 1024)])
        P = 1
        while P < sums.size:
            P *= 2
        want = tree(np.concatenate((sums, np.zeros(P - sums.size))))
        assert ref.tree_sum(v) == want, n


# ------------------------------------------------------------------ the world and the metric
def test_drift_world_is_seeded_and_shaped():
    from sg_pr_amd import metrics, synth
    a, b = synth.drift_world(2), synth.drift_world(2)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert a["rows"].dtype == a["cols"].dtype == a["starts"].dtype == np.int32 and a["T"].shape == (120, 4)
    assert not np.array_equal(a["T"], synth.drift_world(3)["T"])
    assert ((a["rows"] // 300) != (a["cols"] // 300)).all() and np.abs(a["rows"] % 300 - a["cols"] % 300).max() <= 2
    w = synth.drift_world(1, scans=50, sessions=5, closures=40)
    assert w["starts"].tolist() == [0, 50, 100, 150, 200] and w["odom"].shape == (250, 4)
    # closure_world's trajectory was not disturbed by sharing it
    c = synth.closure_world(2)
    assert abs(float(c["Xr"][-1, 2]) - float(np.cumsum(np.cos(np.arctan2(c["Xr"][:, 1], c["Xr"][:, 0])))[-1])) < 1e-9
    # each drive drifts (aligned on its own) and the frames are unrelated (aligned as one map)
    per = metrics.trajectory_error(a["odom"], a["truth"], a["starts"])
    assert per.shape == (2,) and (per > 0.1).all() and (per < 5.0).all()
    assert metrics.trajectory_error(a["odom"], a["truth"]) > 20.0


def test_trajectory_error_is_a_rigid_alignment():
    from sg_pr_amd import metrics
    rng = np.random.default_rng(3)
    xy = rng.normal(size=(50, 2)) * 20.0
    c, s = np.cos(0.7), np.sin(0.7)
    moved = xy @ np.array([[c, s], [-s, c]]) + np.array([5.0, -9.0])
    assert metrics.trajectory_error(moved, xy) < 1e-12
    poses = np.concatenate((np.ones((50, 1)), np.zeros((50, 1)), moved), axis=1)
    assert metrics.trajectory_error(poses, xy) < 1e-12
    bumped = moved.copy()
    bumped[:, 0] += np.where(np.arange(50) % 2, 0.5, -0.5)            # zero mean, uncorrelated with the shape
    assert 0.3 < metrics.trajectory_error(bumped, xy) <= 0.5 + 1e-12
    two = np.concatenate((moved[:25], xy[25:] + 100.0))
    per = metrics.trajectory_error(two, xy, [0, 25])
    assert per.shape == (2,) and per.max() < 1e-12 and metrics.trajectory_error(two, xy) > 1.0
    assert np.isnan(metrics.trajectory_error(xy, xy, [0, 0])[0])
