"""Geometric verification (sgpr_verify_pairs) without a GPU: the C-ABI surface and its argument checks,
and the NumPy definition (tests/geo_ref.py) on planted, mirrored and world-sequence pairs."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ C-ABI surface
def test_symbol_declared_exported_and_abi_version_kept():
    from sg_pr_amd import _build, engine
    header = open(os.path.join(REPO, "include", "sgpr.h")).read()
    assert re.search(r"\bint sgpr_verify_pairs\s*\(", header)
    assert "sgpr_verify_pairs" in engine.ABI_SYMBOLS
    assert "sgpr_verify.hip" in _build.SOURCES
    lib = engine.load_library()
    assert lib.sgpr_verify_pairs is not None
    assert lib.sgpr_abi_version() == 11 == _build.header_abi_version()
    for name, value in (("MAX_NODES", 256), ("INVALID_INDEX", 1), ("NO_HYPOTHESIS", 2), ("TRUNCATED", 4), ("NONFINITE", 8)):
        assert int(re.search(r"#define SGPR_VERIFY_%s (\d+)" % name, header).group(1)) == value
        assert getattr(engine, "VERIFY_" + name) == value
    assert engine.VERIFY_RESULT == geo_ref.RESULT and engine.VERIFY_RESULT.itemsize == 88
    assert [engine.VERIFY_RESULT.fields[n][1] for n in engine.VERIFY_RESULT.names] == [0, 4, 8, 24, 28, 32, 48, 80]


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with NULL or garbage device pointers: had the device been touched,
    the call would have failed with SGPR_E_HIP (no GPU) or crashed (a wild pointer)."""
    from sg_pr_amd import engine
    lib = engine.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    nan = float("nan")

    def call(ca=g, la=g, GA=4, cb=g, lb=g, GB=4, N=100, ia=g, ib=g, P=8, te=0.5, ti=0.6, tz=1.0, mb=5.0, mh=65536, out=g):
        return lib.sgpr_verify_pairs(ca, la, GA, cb, lb, GB, N, ia, ib, P, te, ti, tz, mb, mh, out, None)

    INVALID, NODES = -1, -3
    for name in ("ca", "la", "cb", "lb", "ia", "ib", "out"):
        assert call(**{name: None}) == INVALID, name
        assert b"sgpr_verify_pairs" in lib.sgpr_last_error()
    assert call(P=-1) == INVALID
    for name in ("te", "ti", "tz", "mb"):
        assert call(**{name: -0.5}) == INVALID, name
        assert call(**{name: nan}) == INVALID, name
    assert call(mh=0) == INVALID and call(mh=-7) == INVALID
    for n in (0, -1, 257, 1 << 20):
        assert call(N=n) == NODES, n
    # P == 0 succeeds without a launch, whatever the pointers are
    assert call(P=0) == 0
    assert call(P=0, ca=None, la=None, cb=None, lb=None, ia=None, ib=None, out=None) == 0


# ------------------------------------------------------------------ the definition (tests/geo_ref.py)
def _planted(seed=1, n=40, slots=100, yaw=0.7, t=(3.5, -2.25), labels=6):
    rng = np.random.default_rng(seed)
    ca = np.zeros((slots, 3), np.float32)
    la = -np.ones(slots, np.int32)
    ca[:n, :2] = rng.uniform(-40, 40, (n, 2))
    ca[:n, 2] = rng.uniform(-2, 1, n)
    la[:n] = rng.integers(0, labels, n)
    c, s = np.cos(yaw), np.sin(yaw)
    xy = ca[:n, :2].astype(np.float64)
    bxy = np.stack([c * xy[:, 0] - s * xy[:, 1] + t[0], s * xy[:, 0] + c * xy[:, 1] + t[1]], 1)
    # B: the rotated and translated nodes in permuted slots, padding interleaved
    where = np.sort(rng.choice(slots, n, replace=False))[rng.permutation(n)]
    cb = np.zeros((slots, 3), np.float32)
    lb = -np.ones(slots, np.int32)
    cb[where, :2] = bxy
    cb[where, 2] = ca[:n, 2]
    lb[where] = la[:n]
    return ca, la, cb, lb, where


def test_planted_pair_is_recovered():
    yaw, t = 0.7, (3.5, -2.25)
    ca, la, cb, lb, where = _planted(yaw=yaw, t=t)
    r = geo_ref.verify_pair(ca, la, cb, lb)
    assert r["flags"] == 0 and r["inliers"] == 40 == r["inliers_refined"]
    assert np.abs(r["refined"] - [np.cos(yaw), np.sin(yaw), t[0], t[1]]).max() <= 1e-4
    assert np.abs(r["coarse"] - r["refined"]).max() <= 1e-3 and r["rmse"] <= 1e-4
    i, i2, j, j2 = r["base"]
    assert i < i2 and where[i] == j and where[i2] == j2
    assert r["hypotheses"] >= 1


def test_mirrored_copy_does_not_reach_full_inliers():
    ca, la, _, _, _ = _planted(seed=2)
    cb = ca.copy()
    cb[:, 1] = -cb[:, 1]                       # a reflection is no planar motion
    r = geo_ref.verify_pair(ca, la, cb, la)
    n = int((la >= 0).sum())
    assert r["inliers"] < n and r["inliers_refined"] < n
    assert geo_ref.verify_pair(ca, la, ca, la)["inliers"] == n


def test_flags_of_the_definition():
    ca, la, cb, lb, _ = _planted(seed=3, n=12)
    assert geo_ref.verify_pair(ca, -np.ones_like(la), cb, lb)["flags"] == geo_ref.NO_HYPOTHESIS
    bad = ca.copy()
    bad[3, 1] = np.inf
    r = geo_ref.verify_pair(bad, la, cb, lb)
    assert r["flags"] == geo_ref.NONFINITE and r["inliers"] == 0 and (r["base"] == -1).all() and np.isnan(r["refined"]).all()
    pad = ca.copy()
    pad[50] = np.nan                           # a padding slot may hold anything
    assert geo_ref.verify_pair(pad, la, cb, lb)["flags"] == 0
    r1 = geo_ref.verify_pair(ca, la, cb, lb, max_hyp=1)
    assert r1["flags"] == geo_ref.TRUNCATED and 1 <= r1["hypotheses"] <= 12 * 12
    out = geo_ref.verify_pairs(ca[None], la[None], cb[None], lb[None], [0, -1, 1, 0], [0, 0, 0, 1])
    assert out["flags"].tolist() == [0, 1, 1, 1] and not out[1:].tobytes().strip(b"\0\1")


@pytest.fixture(scope="module")
def world():
    from sg_pr_amd import synth
    return synth.world_sequence(600, 100, seed=0)


def _errors(r, poses, a, b):
    from sg_pr_amd import metrics
    e = metrics.closure_pose_errors({"refined": r["refined"], "flags": r["flags"]}, a, b, poses)
    return e["yaw_deg"], e["trans_m"]


def test_world_revisits_and_non_revisits(world):
    """The 25 true revisits (t, t - 400), t = 400, 408, .., 592, and the 25 non-revisits (t, (t - 250) % 400) of
    world_sequence(600, 100, seed=0) under the default tolerances.
    Bounds (the issue's, about 2x the prototype's extremes): revisits inliers >= 0.7 min(n_real), refined yaw error
    <= 0.5 deg, refined translation error <= 0.2 m; non-revisits inliers <= 8.
    Observed with tests/geo_ref.py: revisits inliers 36 .. 50 (ratio to min(n_real) >= 0.804), refined yaw error
    <= 0.148 deg, refined translation error (Euclidean) <= 0.085 m, hypotheses 1413 .. 5274; non-revisits inliers
    <= 4."""
    centers, labels, n_real, poses = world
    ts = np.arange(400, 600, 8)
    rev = geo_ref.verify_pairs(centers, labels, centers, labels, ts, ts - 400)
    non = geo_ref.verify_pairs(centers, labels, centers, labels, ts, (ts - 250) % 400)
    yaw, trans = _errors(rev, poses, ts, ts - 400)
    ratio = rev["inliers"] / np.minimum(n_real[ts], n_real[ts - 400])
    print("revisits: inliers %d..%d ratio >= %.3f yaw <= %.3f deg trans <= %.3f m hypotheses %d..%d; non-revisits: "
          "inliers <= %d" % (rev["inliers"].min(), rev["inliers"].max(), ratio.min(), yaw.max(), trans.max(),
                             rev["hypotheses"].min(), rev["hypotheses"].max(), non["inliers"].max()))
    assert (rev["flags"] == 0).all()
    assert (ratio >= 0.7).all()
    assert yaw.max() <= 0.5 and trans.max() <= 0.2
    assert (non["inliers"] <= 8).all()
