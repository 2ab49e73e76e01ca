"""The tracking of drives through a landmark map (sgpr_landmark_track, include/sgpr_landmark_track.h)
without a GPU: the C-ABI surface of the ninth header and its argument checks, the NumPy definition
(tests/landmark_track_ref.py) on hand-made cases at every boundary of its rules, mutants of the definition that must each
change an output, and the conditions that make the call worth having, on synth.landmark_world(seed, scans=300): a drive
tracked from one initial pose where dead reckoning and independent alignment fail, and re-acquired after a blackout."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_track_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


# ------------------------------------------------------------------ C-ABI surface
def test_ninth_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, landmarks
    text = open(os.path.join(REPO, "include", "sgpr_landmark_track.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_landmark_track_workspace_bytes", "sgpr_landmark_track"] \
        == landmarks.TRACK_ABI_SYMBOLS
    assert abi.constants == {"SGPR_TRACK_MAX_STAGES": 4, "SGPR_TRACK_START_LOST": 1, "SGPR_TRACK_NONFINITE": 1,
                             "SGPR_TRACK_KEPT": 2, "SGPR_TRACK_LOST": 4, "SGPR_TRACK_NO_ODOM": 8, "SGPR_TRACK_REACQUIRE": 16}
    assert abi.errors == {}
    lib = landmarks.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    (_, r0, a0), (_, r1, a1) = abi.functions
    assert r0 is ctypes.c_size_t and a0 == [ctypes.c_int] * 4
    assert r1 is ctypes.c_int and len(a1) == 31
    ints, doubles = (2, 3, 6, 11, 13, 14, 15, 17, 18, 19, 21), (16, 20)
    assert all(a1[i] is ctypes.c_int for i in ints) and all(a1[i] is ctypes.c_double for i in doubles)
    assert a1[29] is ctypes.c_size_t
    assert all(a1[i] is ctypes.c_void_p for i in range(31) if i not in ints + doubles + (29,))
    # the build lists, and the other eight headers are what they were
    assert "sgpr_landmark_track.hip" in _build.SOURCES and "sgpr_landmark_align.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_landmark_track.h")) for h in _build.HEADERS[1:-1])
    assert any(h.endswith("sgpr_landmark_align_core.hpp") for h in _build.HEADERS)
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any("track" in n for n in engine.ABI_SYMBOLS)
    assert landmarks.ALIGN_ABI_SYMBOLS == ["sgpr_landmark_align_workspace_bytes", "sgpr_landmark_align"]
    assert landmarks.ABI_SYMBOLS == ["sgpr_landmark_workspace_bytes", "sgpr_landmark_map"]
    assert len(landmarks.UPDATE_ABI_SYMBOLS) == 2 and len(landmarks.PERSIST_ABI_SYMBOLS) == 2
    assert (landmarks.TRACK_NONFINITE, landmarks.TRACK_KEPT, landmarks.TRACK_LOST, landmarks.TRACK_NO_ODOM,
            landmarks.TRACK_REACQUIRE) == (ref.NONFINITE, ref.KEPT, ref.LOST, ref.NO_ODOM, ref.REACQUIRE) == (1, 2, 4, 8, 16)
    assert landmarks.TRACK_MAX_STAGES == ref.MAX_STAGES == 4 and landmarks.TRACK_START_LOST == ref.START_LOST == 1


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import landmarks
    lib = landmarks.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    big = 1 << 40
    radius = (ctypes.c_double * 36)(*([0.75] * 36))
    table = (ctypes.c_int32 * 3)(0, 3, 8)

    def call(centers=g, labels=g, Q=8, N=10, odom=g, starts=table, n_tracks=3, init=g, lmc=g, lml=g, use=g, L=20, rad=radius,
             n_stages=3, n_reacquire=1, n_labels=12, tau_z=0.75, iters=3, min_nodes=6, min_matched=10, max_shift=1.0, flags=0,
             out=g, pred=g, node=g, stat=g, rms=g, num=g, ws=g, wsb=big):
        return lib.sgpr_landmark_track(centers, labels, Q, N, odom, starts, n_tracks, init, lmc, lml, use, L, rad, n_stages,
                                       n_reacquire, n_labels, tau_z, iters, min_nodes, min_matched, max_shift, flags, out, pred,
                                       node, stat, rms, num, ws, wsb, None)

    def says(word):
        return b"sgpr_landmark_track" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("centers", "labels", "odom", "init", "lmc", "lml", "out", "pred", "node", "stat", "rms", "num", "ws"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(rad=None) == INVALID and says("h_radius")
    assert call(Q=-1) == INVALID and says("Q ") and call(N=-1) == INVALID and says("N ")
    assert call(L=-1) == INVALID and says("L ") and call(iters=-1) == INVALID and says("iters")
    for ns in (0, -1, 5):
        assert call(n_stages=ns) == INVALID and says("n_stages"), ns
    for nr in (-1, 3, 4):
        assert call(n_reacquire=nr) == INVALID and says("n_reacquire"), nr
    assert call(n_stages=1, n_reacquire=1) == INVALID and says("n_reacquire")
    for mn in (1, 0, -5):
        assert call(min_nodes=mn) == INVALID and says("min_nodes"), mn
    assert call(min_matched=-1) == INVALID and says("min_matched")
    for nl in (0, -1, 65):
        assert call(n_labels=nl) == INVALID and says("n_labels"), nl
    for bad in (-0.5, float("nan")):
        r = (ctypes.c_double * 36)(*([0.75] * 29 + [bad] + [0.75] * 6))
        assert call(rad=r) == INVALID and says("radius of label 5 in stage 2")
        assert call(tau_z=bad) == INVALID and says("tau_z")
        assert call(max_shift=bad) == INVALID and says("max_shift")
    # the track table: NULL with a count, a table without one, a first entry that is not 0, a decreasing entry, one past Q
    assert call(starts=None) == INVALID and says("table") and call(n_tracks=0) == INVALID and says("table")
    assert call(n_tracks=65) == INVALID and call(n_tracks=-1) == INVALID
    for bad_table in ((1, 3, 8), (0, 5, 4), (0, 3, 9)):
        assert call(starts=(ctypes.c_int32 * 3)(*bad_table)) == INVALID and says("table"), bad_table
    assert call(Q=1 << 16, N=1 << 15, starts=None, n_tracks=0) == INVALID and says("int32")
    assert call(Q=0x7fffffff, N=0x7fffffff) == INVALID and says("int32")
    need = lib.sgpr_landmark_track_workspace_bytes(8, 10, 20, 3)
    assert need > 0 and call(wsb=need - 1) == INVALID and says("workspace") and call(wsb=0) == INVALID and says("workspace")
    # Q == 0 or N == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    none = dict(centers=None, labels=None, odom=None, init=None, lmc=None, lml=None, use=None, out=None, pred=None, node=None,
                stat=None, rms=None, num=None, ws=None, wsb=0)
    zero = (ctypes.c_int32 * 3)(0, 0, 0)
    assert call(Q=0, starts=zero) == 0 and call(N=0) == 0 and call(Q=0, starts=zero, **none) == 0 and call(N=0, **none) == 0
    assert call(Q=0, starts=None, n_tracks=0, **none) == 0
    assert call(Q=0, starts=zero, min_nodes=1) == INVALID and call(N=0, iters=-2) == INVALID and call(N=0, L=-1) == INVALID
    assert call(N=0, rad=None) == INVALID and call(N=0, n_labels=0) == INVALID and call(N=0, n_stages=0) == INVALID
    assert call(Q=0) == INVALID and says("table")                # (an entry past Q)


def test_workspace_formula():
    from sg_pr_amd import landmarks
    for Q, N, L in ((1, 1, 0), (1, 1, 1), (2, 64, 11), (300, 100, 512), (300, 100, 513), (4541, 100, 60000), (0, 100, 5), (7, 0, 5),
                    (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1 << 16, 1 << 15, 1)):
        for S in (-1, 0, 1, 2, 3, 4, 5):
            assert landmarks.track_workspace_bytes(Q, N, L, S) == ref.workspace_bytes(Q, N, L, S), (Q, N, L, S)
    # n_stages copies of align's table
    assert ref.workspace_bytes(1, 1, 0, 1) == 1024 * 12 and ref.workspace_bytes(9, 9, 513, 3) == 3 * (2 * 2304 + 2048 * 12)
    assert ref.workspace_bytes(9, 9, 513, 0) == 0 == ref.workspace_bytes(9, 9, 513, 5)
    assert ref.workspace_bytes(9, 9, 513, 4) == 4 * aref.workspace_bytes(9, 9, 513)


# ------------------------------------------------------------------ the rules, on a hand-made drive
se2, drive = ref.se2, ref.hand_drive


def run(d, **kw):
    kw.setdefault("min_nodes", 2)
    kw.setdefault("min_matched", 10)
    kw.setdefault("iters", 3)
    return ref.track(d["centers"], d["labels"], d["odom"], kw.pop("init", d["init"]), kw.pop("lm", d["lm"]),
                     kw.pop("lm_label", d["lm_label"]), kw.pop("lm_use", None), **kw)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_a_tracked_drive_and_a_one_scan_track():
    d = drive()
    out = run(d)
    err = np.hypot(out["poses"][:, 2] - d["truth"][:, 2], out["poses"][:, 3] - d["truth"][:, 3])
    assert err.max() < 0.02 and out["num"].tolist() == [14, 0, 0, 1] and (out["stat"][:, 3] == 0).all()
    assert (out["stat"][:, 0] == 24).all() and (out["stat"][:, 2] == 6).all()
    assert bits(out["pred"][0]) == bits(d["init"][0])
    for i in range(1, 14):
        delta = ref.compose(ref.inverse(d["odom"][i - 1]), d["odom"][i])
        assert bits(out["pred"][i]) == bits(ref.compose(out["poses"][i - 1], delta))
    # a one-scan track is the chained alignment of that scan
    one = {k: (v[:1] if k in ("centers", "labels", "odom") else v) for k, v in d.items()}
    out = run(one)
    X, refits = d["init"], 0
    for r in (2.0, 0.75):
        a = aref.align(d["centers"][:1], d["labels"][:1], X, d["lm"], d["lm_label"], radius=r, iters=3, min_nodes=2)
        X, refits = a["poses"], refits + int(a["stat"][0, 2])
    assert bits(out["poses"]) == bits(X) and bits(out["node_landmark"]) == bits(a["node_landmark"]) and bits(out["rms"]) == bits(a["rms"])
    assert out["stat"].tolist() == [[int(a["stat"][0, 0]), int(a["stat"][0, 1]), refits, 0]] and out["num"].tolist() == [1, 0, 0, 1]


def test_min_matched_at_the_count():
    d = drive()
    use = np.ones(24, np.uint8)
    use[:9] = 0                                                  # 15 landmarks in use: every scan matches 15
    base = run(d, lm_use=use, min_matched=0)
    assert (base["stat"][:, 0] == 15).all()
    keep = run(d, lm_use=use, min_matched=15)
    assert keep["num"].tolist() == [14, 0, 0, 1] and bits(keep["poses"]) == bits(base["poses"])
    lose = run(d, lm_use=use, min_matched=16)
    assert lose["num"].tolist() == [0, 14, 14, 1] and (lose["stat"][:, 3] & ref.LOST).all()
    assert bits(lose["poses"]) == bits(lose["pred"]) and bits(lose["poses"]) != bits(base["poses"])


def test_shift_at_max_shift_and_one_double_below():
    """a shift with dx dx + dy dy == max_shift^2 keeps, the next double of max_shift below loses"""
    d = drive()
    found = 0
    for k in range(40):
        init = ref.compose(d["truth"][0], se2(0.0, 0.2 + 0.01 * k, -0.1))[None]
        free = run(d, init=init)
        dx, dy = free["poses"][0, 2] - init[0, 2], free["poses"][0, 3] - init[0, 3]
        d2 = dx * dx + dy * dy
        s = np.sqrt(d2)
        cand = [v for v in (np.nextafter(s, 0), s, np.nextafter(s, np.inf)) if v * v == d2]
        if not cand:
            continue
        found += 1
        s = cand[0]
        below = np.nextafter(s, 0)
        assert below * below < d2
        at = run(d, init=init, max_shift=s)
        assert not at["stat"][0, 3] & ref.LOST and bits(at["poses"][0]) == bits(free["poses"][0])
        under = run(d, init=init, max_shift=below)
        assert under["stat"][0, 3] & ref.LOST and bits(under["poses"][0]) == bits(init[0])
        assert under["stat"][0, :3].tolist() == free["stat"][0, :3].tolist()       # what the last stage saw is reported all the same
    assert found >= 3
    # +inf disables the test, 0 loses every scan that moved at all
    assert run(d, max_shift=np.inf)["num"][1] == 0 and run(d, max_shift=0.0)["num"][1] == 14


def test_non_finite_odometry_and_init_and_an_empty_track():
    d = drive()
    d["odom"][5, 2] = np.nan
    d["odom"][9, 0] = -np.inf
    out = run(d)
    want = np.zeros(14, np.int64)
    want[[5, 6, 9, 10]] = ref.NO_ODOM                            # non-finite at i, and at i - 1
    assert out["stat"][:, 3].tolist() == want.tolist()
    for i in (5, 6, 9, 10):
        assert bits(out["pred"][i]) == bits(out["poses"][i - 1])
    assert out["num"].tolist() == [14, 0, 0, 1]                  # 0.5 m is inside the 2 m gate: the map pulls the scan back
    # tracks (0..4) (empty) (4..14): the second init is non-finite with a payload; an empty track decides nothing
    d = drive()
    init = np.stack([d["init"][0], se2(0, 99.0, 99.0), d["init"][0]])
    init[2].view(np.uint64)[3] = 0xfff8000000abcdef
    out = run(d, init=init, starts=[0, 4, 4])
    assert out["num"].tolist() == [4, 0, 0, 2]
    assert bits(out["poses"][4:]) == bits(np.tile(init[2], (10, 1))) == bits(out["pred"][4:])
    assert out["stat"][4:].tolist() == [[0, 0, 0, ref.NONFINITE]] * 10 and (out["node_landmark"][4:] == -1).all()
    assert out["rms"][4:].view(np.uint64).tolist() == [0x7ff8000000000000] * 10
    alone = run({k: (v[:4] if k in ("centers", "labels", "odom") else v) for k, v in d.items()})
    assert all(bits(out[k][:4]) == bits(alone[k]) for k in ("poses", "pred", "node_landmark", "stat", "rms"))
    # a second track starts from ITS init, not from the first track's last pose
    init = np.stack([d["init"][0], ref.compose(d["truth"][6], se2(0.0, 0.1, 0.1))])
    out = run(d, init=init, starts=[0, 6])
    assert bits(out["pred"][6]) == bits(init[1]) and out["num"].tolist() == [14, 0, 0, 2]


def test_start_lost_and_reacquire_after_a_lost_scan():
    d = drive()
    radii = (8.0, 2.0, 0.75)
    out = run(d, radii=radii, n_reacquire=1)
    assert (out["stat"][:, 3] == 0).all() and (out["stat"][:, 2] == 6).all()
    out = run(d, radii=radii, n_reacquire=1, flags=ref.START_LOST)
    assert out["stat"][:, 3].tolist() == [ref.REACQUIRE] + [0] * 13 and out["stat"][:, 2].tolist() == [9] + [6] * 13
    assert (run(d, radii=radii, n_reacquire=0, flags=ref.START_LOST)["stat"][:, 2] == 9).all()       # no such stage: three gates each
    # scans 4 and 5 see nothing (labels -1): lost, dead-reckoned; scan 6 runs the wide gate first
    d["labels"][4:6] = -1
    out = run(d, radii=radii, n_reacquire=1)
    fl = out["stat"][:, 3]
    assert fl[4] == ref.LOST | ref.KEPT and fl[5] == ref.LOST | ref.KEPT | ref.REACQUIRE and fl[6] == ref.REACQUIRE
    assert fl[7] == 0 and out["num"].tolist() == [12, 2, 2, 1]
    assert bits(out["poses"][4:6]) == bits(out["pred"][4:6]) and out["stat"][6, 2] == 9


def test_no_landmarks_is_dead_reckoning():
    d = drive()
    out = run(d, lm=np.zeros((0, 3)), lm_label=np.zeros(0, np.int32), radii=(8.0, 2.0, 0.75), n_reacquire=1)
    X = d["init"][0]
    for i in range(14):
        if i:
            X = ref.compose(X, ref.compose(ref.inverse(d["odom"][i - 1]), d["odom"][i]))
        assert bits(out["poses"][i]) == bits(X) == bits(out["pred"][i])
    both = ref.LOST | ref.KEPT
    assert out["stat"].tolist() == [[0, 24, 0, both]] + [[0, 24, 0, both | ref.REACQUIRE]] * 13
    assert out["num"].tolist() == [0, 14, 14, 1] and (out["node_landmark"] == -2).all()
    assert np.hypot(X[2] - d["truth"][13, 2], X[3] - d["truth"][13, 3]) < 0.5      # the odometry here is exact: only init's error
    # min_matched == 0: nothing is ever lost by the count
    out = run(d, lm=np.zeros((0, 3)), lm_label=np.zeros(0, np.int32), min_matched=0)
    assert out["num"].tolist() == [14, 0, 0, 1] and (out["stat"][:, 3] == ref.KEPT).all()


# ------------------------------------------------------------------ mutants of the definition
def test_mutants_change_an_output():
    assert set(ref.MUTANTS) >= {"compose_swapped", "lost_keeps_fit", "reacquire_always", "shift_from_prev", "matched_le",
                                "fused_compose"}
    d = drive()
    use = np.ones(24, np.uint8)
    use[:9] = 0
    cases = {"plain": dict(radii=(8.0, 2.0, 0.75), n_reacquire=1),
             "shift": dict(max_shift=0.45),                                        # a scan moves 0.5 m: more than the gate from A_{i-1}
             "count": dict(lm_use=use, min_matched=15),                            # matched == min_matched on every scan
             "all_lost": dict(min_matched=25)}                                     # lost, though the fit moved the pose
    base = {k: run(d, **kw) for k, kw in cases.items()}
    assert base["shift"]["num"][1] == 0 and base["count"]["num"][1] == 0 and base["all_lost"]["num"][1] == 14
    changed = {}
    for m in ref.MUTANTS:
        changed[m] = sorted(k + ":" + name for k, kw in cases.items() for name, v in run(d, mutant=m, **kw).items()
                            if bits(v) != bits(base[k][name]))
    assert all(changed.values()), changed
    assert "plain:pred" in changed["compose_swapped"] and "plain:pred" in changed["fused_compose"]
    assert "all_lost:poses" in changed["lost_keeps_fit"] and "plain:stat" in changed["reacquire_always"]
    assert "shift:stat" in changed["shift_from_prev"] and "count:num" in changed["matched_le"]
    assert not [c for c in changed["matched_le"] if not c.startswith("count:")]
    again = run(d, mutant=None, **cases["plain"])
    assert all(bits(again[k]) == bits(base["plain"][k]) for k in again)
    with pytest.raises(ValueError):
        run(d, mutant="nope")


# ------------------------------------------------------------------ the conditions, on the reference alone
planted = ref.planted_drive


def trans_err(X, truth):
    return np.hypot(X[:, 2] - truth[:, 2], X[:, 3] - truth[:, 3])


def tracked(p, use, reacquire):
    return ref.track(p["centers"], p["labels"], p["odom"], p["init"], p["lm"]["center"], p["lm"]["label"], use,
                     radii=((8.0,) if reacquire else ()) + (2.0, 0.75), n_reacquire=int(reacquire), iters=10, min_nodes=6,
                     min_matched=10)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_tracking_follows_a_drive_that_dead_reckoning_and_independent_alignment_lose(seed):
    p = planted(seed)
    truth = p["truth"]
    out = tracked(p, p["use"], False)
    err, dead = trans_err(out["poses"], truth), trans_err(p["dead"], truth)
    Z = p["dead"]
    for r in (2.0, 0.75):
        Z = aref.align(p["centers"], p["labels"], Z, p["lm"]["center"], p["lm"]["label"], p["use"], radius=r, iters=10,
                       min_nodes=6)["poses"]
    off = int((trans_err(Z, truth) > 0.5).sum())
    print("seed %d: dead reckoning %.2f / %.2f m (median / max); independent alignment from it: %d of 300 beyond 0.5 m; tracked "
          "%.3f / %.3f / %.3f m (median / 95 %% / max), lost %d"
          % (seed, np.median(dead), dead.max(), off, np.median(err), np.percentile(err, 95), err.max(), out["num"][1]))
    assert err.max() < 0.2 and np.median(err) < 0.05
    assert out["num"].tolist() == [300, 0, 0, 1] and not (out["stat"][:, 3] & ref.LOST).any()
    if seed in (0, 2, 3):
        assert off >= 50                                          # what tracking is for


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_blackout_is_dead_reckoned_through_and_the_track_re_acquired(seed):
    p = planted(seed)
    truth = p["truth"]
    out = tracked(p, p["blackout"], True)
    lost = (out["stat"][:, 3] & ref.LOST) != 0
    err = trans_err(out["poses"], truth)
    print("seed %d: blackout: lost %d scans (%d..%d, longest run %d); not lost: max %.3f m; last 20 scans: max %.3f m"
          % (seed, lost.sum(), np.flatnonzero(lost).min(), np.flatnonzero(lost).max(), out["num"][2], err[~lost].max(),
             err[-20:].max()))
    assert 60 <= lost.sum() <= 100 and out["num"][1] == lost.sum() and out["num"][0] == 300 - lost.sum()
    assert bits(out["poses"][lost]) == bits(out["pred"][lost])
    assert err[~lost].max() < 0.3 and err[-20:].max() < 0.2 and not lost[-20:].any()
    if seed in (0, 3):
        narrow = tracked(p, p["blackout"], False)
        gone = (narrow["stat"][:, 3] & ref.LOST) != 0
        print("seed %d: without the 8 m stage: lost %d scans, scan 299 off by %.2f m" % (seed, gone.sum(), trans_err(narrow["poses"], truth)[299]))
        assert gone[299]                                          # still lost at the end: what the stage is for
