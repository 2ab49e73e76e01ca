"""The relocalisation of scans in a landmark map (sgpr_landmark_relocalize, include/sgpr_landmark_relocalize.h,
DESIGN.md §35) without a GPU: the C-ABI surface of the tenth header and its argument checks, the NumPy definition
(tests/landmark_relocalize_ref.py) on hand-made cases at every boundary of its rules, mutants of the definition that
must each change an output, the aliased map, and the conditions that make the call worth having, on
synth.landmark_world(seed, scans=300): scans of a third drive placed in the map of the first two with no pose at all."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_relocalize_ref as ref  # noqa: E402
import landmark_track_ref as tref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
run, up, down = ref.run, ref.up, ref.down


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------ C-ABI surface
def test_tenth_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, landmarks
    text = open(os.path.join(REPO, "include", "sgpr_landmark_relocalize.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_landmark_relocalize_workspace_bytes", "sgpr_landmark_relocalize"] \
        == landmarks.RELOCALIZE_ABI_SYMBOLS
    assert abi.constants == {"SGPR_RELOC_MAX_STAGES": 16, "SGPR_RELOC_FOUND": 1, "SGPR_RELOC_KEPT": 2, "SGPR_RELOC_TRUNCATED": 4,
                             "SGPR_RELOC_NO_HYPOTHESIS": 8}
    assert abi.errors == {}
    lib = landmarks.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    (_, r0, a0), (_, r1, a1) = abi.functions
    assert r0 is ctypes.c_size_t and a0 == [ctypes.c_int] * 4
    assert r1 is ctypes.c_int and len(a1) == 33
    ints, doubles = (2, 3, 7, 10, 11, 16, 17, 19, 20), (12, 13, 14, 15, 18)
    assert all(a1[i] is ctypes.c_int for i in ints) and all(a1[i] is ctypes.c_double for i in doubles)
    assert a1[31] is ctypes.c_size_t
    assert all(a1[i] is ctypes.c_void_p for i in range(33) if i not in ints + doubles + (31,))
    # the build lists, and the other nine headers are what they were
    assert "sgpr_landmark_relocalize.hip" in _build.SOURCES and "sgpr_landmark_track.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_landmark_relocalize.h")) for h in _build.HEADERS[1:-1])
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any("relocalize" in n for n in engine.ABI_SYMBOLS)
    counts = {"sgpr_posegraph.h": 2, "sgpr_localize.h": 1, "sgpr_landmarks.h": 2, "sgpr_landmark_refine.h": 2,
              "sgpr_landmark_align.h": 2, "sgpr_landmark_update.h": 2, "sgpr_landmark_persist.h": 2, "sgpr_landmark_track.h": 2}
    for name, n in counts.items():
        assert len(engine.public_header(name).functions) == n, name
    assert landmarks.TRACK_ABI_SYMBOLS == ["sgpr_landmark_track_workspace_bytes", "sgpr_landmark_track"]
    assert (landmarks.RELOC_FOUND, landmarks.RELOC_KEPT, landmarks.RELOC_TRUNCATED, landmarks.RELOC_NO_HYPOTHESIS) \
        == (ref.FOUND, ref.KEPT, ref.TRUNCATED, ref.NO_HYPOTHESIS) == (1, 2, 4, 8)
    assert landmarks.RELOC_MAX_STAGES == ref.MAX_STAGES == 16


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import landmarks
    lib = landmarks.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    big = 1 << 40
    rin = (ctypes.c_double * 12)(*([0.75] * 12))
    radii = (ctypes.c_double * 36)(*([0.75] * 36))

    def call(centers=g, labels=g, Q=8, N=10, lmc=g, lml=g, use=g, L=20, rin=rin, rad=radii, n_stages=3, n_labels=12, tau_z=0.75,
             tau_edge=0.5, min_base=5.0, max_base=30.0, max_hyp=100, min_inliers=12, sep=10.0, iters=3, min_nodes=6, out=g, coarse=g,
             other=g, node=g, stat=g, win=g, hyp=g, rms=g, num=g, ws=g, wsb=big):
        return lib.sgpr_landmark_relocalize(centers, labels, Q, N, lmc, lml, use, L, rin, rad, n_stages, n_labels, tau_z, tau_edge,
                                            min_base, max_base, max_hyp, min_inliers, sep, iters, min_nodes, out, coarse, other, node,
                                            stat, win, hyp, rms, num, ws, wsb, None)

    def says(word):
        return b"sgpr_landmark_relocalize" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("centers", "labels", "lmc", "lml", "out", "coarse", "other", "node", "stat", "win", "hyp", "rms", "num", "ws"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(rin=None) == INVALID and says("h_radius_in") and call(rad=None) == INVALID and says("h_radii")
    assert call(Q=-1) == INVALID and says("Q ") and call(N=-1) == INVALID and says("N ")
    assert call(L=-1) == INVALID and says("L ") and call(iters=-1) == INVALID and says("iters")
    for ns in (-1, 17):
        assert call(n_stages=ns) == INVALID and says("n_stages"), ns
    for nl in (0, -1, 65):
        assert call(n_labels=nl) == INVALID and says("n_labels"), nl
    for bad in (-0.5, float("nan")):
        r = (ctypes.c_double * 36)(*([0.75] * 29 + [bad] + [0.75] * 6))
        assert call(rad=r) == INVALID and says("radius of label 5 in stage 2")
        r = (ctypes.c_double * 12)(*([0.75] * 7 + [bad] + [0.75] * 4))
        assert call(rin=r) == INVALID and says("inlier radius of label 7")
        for name in ("tau_z", "tau_edge", "min_base", "sep"):
            assert call(**{name: bad}) == INVALID and says(name), name
        assert call(max_base=bad) == INVALID and says("max_base")
    assert call(max_base=4.9) == INVALID and says("max_base") and call(max_base=float("inf")) == INVALID and says("max_base")
    for v in (0, -3):
        assert call(max_hyp=v) == INVALID and says("max_hyp")
    for v in (1, 0, -5):
        assert call(min_inliers=v) == INVALID and says("min_inliers") and call(min_nodes=v) == INVALID and says("min_nodes")
    assert call(Q=1 << 16, N=1 << 15) == INVALID and says("int32") and call(Q=0x7fffffff, N=0x7fffffff) == INVALID and says("int32")
    need = lib.sgpr_landmark_relocalize_workspace_bytes(8, 10, 20, 3)
    assert need > 0 and call(wsb=need - 1) == INVALID and says("workspace") and call(wsb=0) == INVALID and says("workspace")
    # what is legal: +inf tolerances and radii, sep = +inf, min_base == max_base, no stage without a stage table - each
    # gets past the value checks and stops at the next fault, the short workspace
    inf = float("inf")
    for kw in (dict(tau_z=inf), dict(tau_edge=inf), dict(sep=inf), dict(min_base=5.0, max_base=5.0), dict(n_stages=0, rad=None),
               dict(rin=(ctypes.c_double * 12)(*([inf] * 12))), dict(L=0, lmc=None, lml=None, use=None), dict(use=None)):
        assert call(wsb=0, **kw) == INVALID and says("workspace"), kw
    # Q == 0 or N == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    none = dict(centers=None, labels=None, lmc=None, lml=None, use=None, out=None, coarse=None, other=None, node=None, stat=None,
                win=None, hyp=None, rms=None, num=None, ws=None, wsb=0)
    assert call(Q=0) == 0 and call(N=0) == 0 and call(Q=0, **none) == 0 and call(N=0, **none) == 0
    assert call(Q=0, min_nodes=1) == INVALID and call(N=0, iters=-2) == INVALID and call(N=0, L=-1) == INVALID
    assert call(N=0, rin=None) == INVALID and call(N=0, n_labels=0) == INVALID and call(N=0, n_stages=17) == INVALID
    assert call(Q=0, max_hyp=0) == INVALID and call(Q=0, sep=-1.0) == INVALID


def test_workspace_formula():
    from sg_pr_amd import landmarks
    for Q, N, L in ((1, 1, 0), (1, 1, 1), (2, 64, 11), (300, 100, 512), (300, 100, 513), (4541, 100, 60000), (3, 256, 9), (3, 257, 9),
                    (0, 100, 5), (7, 0, 5), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1 << 16, 1 << 15, 1)):
        for S in (-1, 0, 1, 2, 16, 17):
            assert landmarks.relocalize_workspace_bytes(Q, N, L, S) == ref.workspace_bytes(Q, N, L, S), (Q, N, L, S)
    t = aref.workspace_bytes(9, 9, 513)
    assert ref.workspace_bytes(9, 9, 513, 0) == 2 * t + 512 and ref.workspace_bytes(9, 9, 513, 3) == 5 * t + 512 + 3 * 512
    assert ref.workspace_bytes(3, 257, 9, 1) - ref.workspace_bytes(3, 256, 9, 1) == 3328      # 3 x 257 x 4 = 3084, rounded up to 256
    assert ref.workspace_bytes(9, 9, 513, 17) == 0 == ref.workspace_bytes(9, 9, 513, -1)


# ------------------------------------------------------------------ the rules, on hand-made worlds
def flags(o, q=0):
    return int(o["stat"][q, 5])


def test_the_identity_hypothesis_with_every_threshold_met_exactly():
    ex = ref.exact_world()
    o = run(ex)
    # (A', B') on (A, B): c = 100 / 100, s = 0 / 100, midpoint on midpoint - the identity, bit for bit
    assert o["coarse"][0].tolist() == [1.0, 0.0, 0.0, 0.0] == o["poses"][0].tolist() and o["win"][0].tolist() == [0, 1, 0, 1]
    assert o["stat"][0].tolist() == [5, 2, 5, 5, 0, ref.FOUND, 2, 0] and o["hyp"][0] == 16 and o["num"].tolist() == [1, 0, 0, 0]
    assert o["node_landmark"][0].tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and o["rms"][0] == np.sqrt(0.5625 / 5.0)
    # one double past each threshold
    for name in ("min_base_past", "max_base_past"):
        w, over = ref.hand_cases()[name]
        p = run(w, **over)
        assert flags(p) == ref.NO_HYPOTHESIS and p["hyp"][0] == 0 and p["stat"][0, 6] == 0 and p["win"][0].tolist() == [-1] * 4
        assert p["coarse"].view(np.uint64).tolist() == [[0x7ff8000000000000] * 4] == p["poses"].view(np.uint64).tolist()
        assert p["node_landmark"][0].tolist() == [-2] * 5 + [-1] * 3 and p["num"].tolist() == [0, 0, 1, 0]
    for name in ("min_base_at_wide", "max_base_at_wide"):
        w, over = ref.hand_cases()[name]
        assert all(bits(run(w, **over)[k]) == bits(o[k]) for k in o)
    assert run(ex, tau_edge=down(0.5))["hyp"][0] == 12           # (E, F), 10.5 apart, no longer pairs with a base of 10
    z = run(ex, tau_z=down(0.75))
    assert z["hyp"][0] == 8 and z["win"][0].tolist() == [2, 3, 2, 3] and z["stat"][0, 0] == 3 and not flags(z) & ref.FOUND
    # only landmark A (under node i), or only B (under node i'), one double outside tau_z: either kills (A', B', A, B)
    for name in ("tau_z_j_only", "tau_z_jp_only"):
        w, over = ref.hand_cases()[name]
        h = run(w, **over)
        assert h["hyp"][0] == 12 and h["win"][0].tolist() == [2, 3, 2, 3] and h["stat"][0, 0] == 4
        assert run(ex, **over)["hyp"][0] == 16 and run(ex, **over)["win"][0].tolist() == [0, 1, 0, 1]
    r = run(ex, radius_in=down(0.75))
    assert r["stat"][0, 0] == 4 and r["hyp"][0] == 16 and not flags(r) & ref.FOUND and np.isnan(r["poses"]).all()
    assert run(ex, radius_in=down(0.75), min_inliers=4)["node_landmark"][0].tolist() == [0, 1, 2, 3, -2, -1, -1, -1]
    # min_inliers met, and one fewer
    m = run(ex, min_inliers=6)
    assert flags(m) == 0 and m["stat"][0].tolist() == [5, 0, 0, 5, 0, 0, 2, 0] and bits(m["coarse"]) == bits(o["coarse"])
    assert np.isnan(m["other"]).all() and m["num"].tolist() == [0, 0, 0, 0] and m["rms"].view(np.uint64)[0] == 0x7ff8000000000000
    # stages from the coarse pose: two gates of three steps each
    s = run(ex, radii=(2.0, 0.75), iters=3)
    assert s["stat"][0, 4] == 6 and bits(s["coarse"]) == bits(o["coarse"]) and flags(s) == ref.FOUND


def test_den_must_be_positive():
    """two coincident landmarks (lv = 0) under two nodes a quarter metre apart, and two coincident nodes (lu = 0) with
    min_base = 0: the edge test passes, den = 0 does not - no NaN pose is ever evaluated"""
    w, over = ref.hand_cases()["coincident"]
    o = run(w, **over)
    assert o["stat"][0, 6] == 6 and np.isfinite(o["coarse"]).all() and np.isfinite(o["other"]).all()
    assert o["hyp"][0] == 20 and not {9, 10} & set(o["win"][0, 2:].tolist())
    assert run(w, **dict(over, tau_edge=20.0))["hyp"][0] > 20 and np.isfinite(run(w, **dict(over, tau_edge=20.0))["coarse"]).all()


def test_separation_at_the_distance_and_one_double_below():
    la = ref.lattice_world()
    o = run(la)
    assert o["win"][0].tolist() == [0, 1, 0, 6] and o["coarse"][0].tolist() == [1.0, 0.0, 0.0, 0.0] and o["stat"][0, :2].tolist() == [4, 4]
    at, past = run(la, sep=8.0), run(la, sep=down(8.0))
    d_at = np.hypot(at["other"][0, 2], at["other"][0, 3])
    d_past = np.hypot(past["other"][0, 2], past["other"][0, 3])
    assert d_past == 8.0 and d_at > 8.0 and at["stat"][0, 1] == past["stat"][0, 1] == 4
    assert run(la, sep=0.0)["stat"][0, 1] == 4 and np.hypot(*run(la, sep=0.0)["other"][0, 2:]) > 0.0
    inf = run(la, sep=np.inf)
    assert inf["stat"][0, 1] == 0 and inf["other"].view(np.uint64).tolist() == [[0x7ff8000000000000] * 4]


def test_ties_go_to_the_lowest_key_on_a_lattice():
    la = ref.lattice_world()
    o = run(la)
    # 25 translates x 4 quarter turns of the block score 4 like the truth: the winner is the first of them by (i, i', j, j')
    assert o["win"][0].tolist() == [0, 1, 0, 6] and o["hyp"][0] == 680
    hi = run(la, mutant="ties_high")
    assert hi["win"][0].tolist() != o["win"][0].tolist() and hi["stat"][0, 0] == 4
    # renumbering the landmarks moves the winner with the numbers
    perm = np.random.default_rng(1).permutation(36)
    w = dict(la)
    w["lm"] = la["lm"][perm]
    p = run(w)
    assert p["stat"][0, 0] == 4 and p["win"][0, :2].tolist() == [0, 1] and p["win"][0, 2] == 0


def test_the_cap_stops_before_a_base_pair_never_inside_one():
    la = ref.lattice_world()
    free = run(la)
    caps, m = [], 1
    while True:
        o = run(la, max_hyp=m)
        caps.append(int(o["hyp"][0]))
        if not flags(o) & ref.TRUNCATED:
            break
        m = caps[-1] + 1
    assert len(caps) == 6 and caps[-1] == 680 == free["hyp"][0] and caps == sorted(set(caps))
    for k, c in enumerate(caps):
        at, past = run(la, max_hyp=c), run(la, max_hyp=c + 1)
        assert at["hyp"][0] == c and at["stat"][0, 6] == k + 1
        # reached by the last base pair: nothing was left out, nothing is flagged
        assert bool(flags(at) & ref.TRUNCATED) == (k < 5) and at["num"][1] == int(k < 5)
        assert past["hyp"][0] == caps[min(k + 1, 5)] and past["stat"][0, 6] == min(k + 2, 6)
    cut = run(la, max_hyp=caps[0], mutant="cap_inside")
    assert cut["hyp"][0] == caps[0] and run(la, max_hyp=caps[0] - 1, mutant="cap_inside")["hyp"][0] == caps[0] - 1
    assert run(la, max_hyp=caps[0] - 1)["hyp"][0] == caps[0]


def test_few_landmarks_few_nodes_dead_labels_and_nans():
    cases = ref.hand_cases()
    for L in (0, 1):
        o = run(*cases["L%d" % L][:1], **cases["L%d" % L][1])
        assert flags(o) == ref.NO_HYPOTHESIS and o["stat"][0].tolist() == [0, 0, 0, 5, 0, 8, 2, 0] and o["num"].tolist() == [0, 0, 1, 0]
    o = run(cases["L2"][0], **cases["L2"][1])
    assert o["hyp"][0] == 4 and o["stat"][0, :3].tolist() == [2, 0, 2] and o["win"][0].tolist() == [0, 1, 0, 1]
    o = run(cases["one_live_node"][0])
    assert flags(o) == ref.NO_HYPOTHESIS and o["stat"][0, 3] == 1 and o["stat"][0, 6] == 0 and o["node_landmark"][0].tolist() == [-2] + [-1] * 7
    # a label of radius 0 is dead on both sides: its nodes are -1, its landmarks take no part
    o = run(cases["radius_zero"][0], **cases["radius_zero"][1])
    assert o["stat"][0, 3] == 2 and o["node_landmark"][0].tolist() == [0, 1, -1, -1, -1, -1, -1, -1] and o["stat"][0, 6] == 1
    o = run(cases["stage_radius_zero"][0], **cases["stage_radius_zero"][1])
    assert o["stat"][0, 3] == 5 and o["stat"][0, 4] == 4
    n = run(cases["nan_node"][0], **cases["nan_node"][1])
    assert n["node_landmark"][0, 2] == -1 and n["stat"][0, 3] == 4 and n["stat"][0, 6] == 1 and np.isfinite(n["poses"]).all()
    lmn = run(cases["nan_landmark"][0], **cases["nan_landmark"][1])
    assert lmn["node_landmark"][0, 2] == -2 and lmn["stat"][0, :4].tolist() == [4, 2, 4, 5] and lmn["hyp"][0] == 12
    pad = run(cases["nan_padding"][0], **cases["nan_padding"][1])
    base = run(ref.exact_world(), min_inliers=3)
    assert all(bits(pad[k]) == bits(base[k]) for k in base)


def test_scans_are_independent_and_the_count_is_the_alignment_count():
    ex, la = ref.exact_world(), ref.lattice_world()
    both = ref.relocalize(np.concatenate((ex["centers"], la["centers"], ex["centers"])), np.concatenate((ex["labels"], la["labels"], ex["labels"])),
                          ex["lm"], ex["lm_label"], **dict(ex["kw"], min_inliers=4))
    one = run(ex, min_inliers=4)
    assert all(bits(both[k][0]) == bits(one[k][0]) == bits(both[k][2]) for k in one if k != "num") and both["num"][0] >= 2
    # the inliers of a hypothesis ARE `matched` of the alignment with iters = 0 from its pose: on every hypothesis of the
    # dense world's first base pairs, through the grid path of the reference and without it
    w = ref.dense_world()
    rng = np.random.default_rng(3)
    poses = np.stack([ref.se2(a, x, y) for a, x, y in zip(rng.uniform(-3, 3, 400), rng.uniform(-5, 40, 400), rng.uniform(-5, 40, 400))])
    poses[0] = w["truth"]
    cen, lab = w["centers"][0], w["labels"][0]
    live = lab >= 0
    x, y, z = (cen[live, k].astype(np.float64) for k in range(3))
    elab = aref.eligible(w["lm"], w["lm_label"], None, np.full(1, 0.5))
    got = ref.count_inliers(poses, x, y, z, lab[live].astype(np.int64), w["lm"], elab, np.full(1, 0.5), np.float64(0.75))
    al = aref.align(np.repeat(w["centers"], 400, 0), np.repeat(w["labels"], 400, 0), poses, w["lm"], w["lm_label"], radius=0.5, iters=0,
                    n_labels=1)
    assert got.tolist() == al["stat"][:, 0].tolist() and got[0] == 6 and 0 < (got > 0).sum() < 400
    old = ref._CHUNK
    try:
        ref._CHUNK = 1 << 10
        assert ref.count_inliers(poses, x, y, z, lab[live].astype(np.int64), w["lm"], elab, np.full(1, 0.5), np.float64(0.75)).tolist() == got.tolist()
    finally:
        ref._CHUNK = old


# ------------------------------------------------------------------ mutants of the definition
def test_mutants_change_an_output():
    assert set(ref.MUTANTS) >= {"min_base_lt", "max_base_lt", "tau_edge_lt", "tau_z_lt", "radius_lt", "sep_ge", "min_inliers_gt",
                                "no_height", "from_node_i", "ties_high", "cap_inside", "sep_refined", "fused_c", "refine_unfound",
                                "height_i_only", "height_ip_only"}
    ex = ref.exact_world()
    cases = ref.mutant_cases()
    base = {k: run(w, **kw) for k, (w, kw) in cases.items()}
    changed = {}
    for m in ref.MUTANTS:
        changed[m] = sorted(k + ":" + name for k, (w, kw) in cases.items() for name, v in run(w, mutant=m, **kw).items()
                            if bits(v) != bits(base[k][name]))
    assert all(changed.values()), changed
    for m in ("min_base_lt", "max_base_lt", "tau_edge_lt", "tau_z_lt"):
        assert "exact:hyp" in changed[m], m
    assert "exact:stat" in changed["radius_lt"] and "exact:hyp" not in changed["radius_lt"]
    assert "lattice_sep:other" in changed["sep_ge"] and "exact:stat" in changed["min_inliers_gt"]
    assert "high:hyp" in changed["no_height"] and "exact:hyp" not in changed["no_height"]
    assert "exact:coarse" not in changed["from_node_i"] and "tilt:coarse" in changed["from_node_i"]
    assert "lattice:win" in changed["ties_high"] and "lattice_cap:hyp" in changed["cap_inside"]
    assert "turned:coarse" in changed["fused_c"] and "unfound:poses" in changed["refine_unfound"]
    sh = base["shifted"]
    assert sh["coarse"][0].tolist() == [1.0, 0.0, 0.0, 0.0] and sh["poses"][0, 2] < -0.05 and sh["stat"][0, 4] > 0
    assert "shifted:other" in changed["sep_refined"] and not [c for c in changed["sep_refined"] if not c.startswith("shifted:")]
    # a height test on one base node only lets (A', B', A, B) back in - and win - in the world where only the OTHER
    # node's landmark is out
    assert "height_jp:win" in changed["height_i_only"] and "height_j:win" not in changed["height_i_only"]
    assert "height_j:win" in changed["height_ip_only"] and "height_jp:win" not in changed["height_ip_only"]
    with pytest.raises(ValueError):
        run(ex, mutant="nope")


# ------------------------------------------------------------------ the aliased map
def test_the_aliased_map_is_seen_as_ambiguous():
    al = ref.aliased_map()
    w, _ = ref.hand_cases()["aliased"]
    o = run(w)
    n, gap = al["n"], al["gap"]
    assert flags(o) & ref.FOUND and o["stat"][0, 0] == n == 14 and o["stat"][0, 1] == n - 1
    assert (o["win"][0, 2:] < n).all() and (o["node_landmark"][0] == np.arange(n)).all()          # the complete copy
    assert np.hypot(*(o["poses"][0, 2:] - al["truth"][2:])) < 0.05
    assert abs(o["other"][0, 2] - o["coarse"][0, 2] - gap) < 1e-9 and abs(o["other"][0, 3] - o["coarse"][0, 3]) < 1e-9
    assert o["stat"][0, 1] >= 0.7 * o["stat"][0, 0]                                               # ambiguous at the default ratio
    masked = run(*ref.hand_cases()["aliased_masked"][:1], **ref.hand_cases()["aliased_masked"][1])
    # (0 is out of reach under the definition: a hypothesis elsewhere counts at least the base nodes it was made from, and
    #  here a third node falls on a landmark by chance)
    assert bits(masked["poses"]) == bits(o["poses"]) and masked["stat"][0, 0] == n and masked["stat"][0, 1] == 3
    # with the first copy masked out instead, the incomplete copy is the answer
    use = np.ones(2 * n - 1, np.uint8)
    use[:n] = 0
    second = run(w, lm_use=use)
    assert second["stat"][0, 0] == n - 1 and abs(second["poses"][0, 2] - o["poses"][0, 2] - gap) < 0.05


# ------------------------------------------------------------------ the conditions, on the reference alone
QUERY = np.arange(0, 300, 10)
# measured with this reference: every seed finds 30 of 30 within 0.5 m; the worst median / 95 % / max
# error of a found scan is WORST below
WORST = {"found_within": 1.0, "median": 0.034, "p95": 0.071, "max": 0.076}


@pytest.fixture(scope="module")
def planted():
    out = {}
    for seed in range(4):
        p = tref.planted_drive(seed)
        args = (p["centers"][QUERY], p["labels"][QUERY], p["lm"]["center"], p["lm"]["label"], p["use"])
        out[seed] = (p, args, ref.relocalize(*args))
    return out


def errors(o, truth):
    return np.hypot(o["poses"][:, 2] - truth[:, 2], o["poses"][:, 3] - truth[:, 3])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scans_of_a_third_drive_are_placed_with_no_pose(planted, seed):
    p, args, o = planted[seed]
    truth = p["truth"][QUERY]
    err, st = errors(o, truth), o["stat"]
    found = (st[:, 5] & ref.FOUND) != 0
    within = found & (err < 0.5)
    amb = found & (st[:, 1] >= 0.7 * st[:, 0])
    print("seed %d: found %.3f, within 0.5 m %.3f; error of the found %.3f / %.3f / %.3f m (median / 95 %% / max); inliers %d / %d, "
          "other %d / %d (median / max); hypotheses %d / %d; ambiguous %d"
          % (seed, found.mean(), within.mean(), np.median(err[found]), np.percentile(err[found], 95), err[found].max(),
             np.median(st[:, 0]), st[:, 0].max(), np.median(st[:, 1]), st[:, 1].max(), np.median(o["hyp"]), o["hyp"].max(), amb.sum()))
    assert within.mean() >= WORST["found_within"] - 0.05
    assert np.median(err[found]) <= 1.5 * WORST["median"] and np.percentile(err[found], 95) <= 1.5 * WORST["p95"]
    assert err[found].max() <= 1.5 * WORST["max"]
    assert not (found & ~amb & (err > 1.0)).any()
    # as good as the alignment from a good init: the truth displaced by 0.3 m
    rng = np.random.default_rng(70 + seed)
    ang = rng.uniform(0, 2 * np.pi, QUERY.size)
    X = np.stack([tref.compose(t, ref.se2(0.0, 0.3 * np.cos(a), 0.3 * np.sin(a))) for t, a in zip(truth, ang)])
    for r in (2.0, 0.75):
        X = aref.align(args[0], args[1], X, args[2], args[3], args[4], radius=r)["poses"]
    good = np.hypot(X[:, 2] - truth[:, 2], X[:, 3] - truth[:, 3])
    print("seed %d: aligned from the truth + 0.3 m: %.3f / %.3f m (median / max)" % (seed, np.median(good[found]), good[found].max()))
    assert np.median(err[found]) <= 1.5 * np.median(good[found]) and err[found].max() <= 1.5 * good[found].max()
    # truncation is benign
    cut = ref.relocalize(*args, max_hyp=4096)
    cerr = errors(cut, truth)
    cfound = (cut["stat"][:, 5] & ref.FOUND) != 0
    assert (cfound & (cerr < 0.5)).mean() >= WORST["found_within"] - 0.05
    low = ref.relocalize(*args, max_hyp=100)
    lfound = (low["stat"][:, 5] & ref.FOUND) != 0
    print("seed %d: max_hyp 100: truncated %d, found within 0.5 m %.3f" % (seed, ((low["stat"][:, 5] & ref.TRUNCATED) != 0).sum(),
                                                                             (lfound & (errors(low, truth) < 0.5)).mean()))
    assert ((low["stat"][:, 5] & ref.TRUNCATED) != 0).all() and (lfound & (errors(low, truth) < 0.5)).mean() >= WORST["found_within"] - 0.05
