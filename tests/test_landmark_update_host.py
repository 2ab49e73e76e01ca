"""The incremental update of a landmark map (sgpr_landmark_update, include/sgpr_landmark_update.h) without
a GPU: the C-ABI surface of the seventh header and its argument checks, the NumPy definition
(tests/landmark_update_ref.py) on hand-made cases at every boundary of its rules and on synth.landmark_world - the map of
two drives, the third aligned to it and folded in, set against the batch map of all three - and mutants of the definition
that must each change an output."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_ref as lref  # noqa: E402
import landmark_update_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
IDENT = (1.0, 0.0, 0.0, 0.0)
F32 = np.float32


def lm_of(center, label, count=None, first=None, sessions=None, spread=None):
    n = len(label)
    return {"center": np.array(center, np.float64).reshape(-1, 3), "label": np.array(label, np.int32),
            "count": np.array([1] * n if count is None else count, np.int32),
            "first": np.array(list(range(n)) if first is None else first, np.int32),
            "sessions": np.array([1] * n if sessions is None else sessions, np.uint64),
            "spread": np.array([0.0] * n if spread is None else spread, np.float64)}


def one(nodes, labels, assoc, lm, pose=IDENT, **kw):
    """one scan through the reference"""
    return ref.update(np.array([nodes], F32), np.array([labels], np.int32), np.array([pose], np.float64),
                      np.array([assoc], np.int32), lm, **kw)


def same_record(out, lm, i):
    return all(np.asarray(out[k][i]).tobytes() == np.asarray(lm[k][i]).tobytes() for k in ref.RECORD)


# ------------------------------------------------------------------ C-ABI surface
def test_seventh_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, landmarks, localize, posegraph
    text = open(os.path.join(REPO, "include", "sgpr_landmark_update.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_landmark_update_workspace_bytes", "sgpr_landmark_update"] \
        == landmarks.UPDATE_ABI_SYMBOLS
    assert abi.constants == {} and abi.errors == {}
    lib = landmarks.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    (_, r0, a0), (_, r1, a1) = abi.functions
    assert r0 is ctypes.c_size_t and a0 == [ctypes.c_int] * 3
    assert r1 is ctypes.c_int and len(a1) == 32
    ints = (2, 3, 7, 8, 9, 11, 19, 20)
    assert [a1[i] for i in ints] == [ctypes.c_int] * 8
    assert a1[12] is ctypes.c_double and a1[30] is ctypes.c_size_t
    assert all(a1[i] is ctypes.c_void_p for i in range(32) if i not in ints + (12, 30))
    # the build lists, and the other six headers are what they were
    assert "sgpr_landmark_update.hip" in _build.SOURCES and "sgpr_landmarks.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_landmark_update.h")) for h in _build.HEADERS[1:-1])
    assert any(h.endswith("sgpr_landmark_core.hpp") for h in _build.HEADERS[1:-1])
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any("update" in n and "landmark" in n for n in engine.ABI_SYMBOLS)
    assert landmarks.ABI_SYMBOLS == ["sgpr_landmark_workspace_bytes", "sgpr_landmark_map"]
    assert landmarks.REFINE_ABI_SYMBOLS == ["sgpr_landmark_refine_workspace_bytes", "sgpr_landmark_refine"]
    assert landmarks.ALIGN_ABI_SYMBOLS == ["sgpr_landmark_align_workspace_bytes", "sgpr_landmark_align"]
    assert len(posegraph.ABI_SYMBOLS) == 2 and localize.ABI_SYMBOLS == ["sgpr_localize_scans"]


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import landmarks
    lib = landmarks.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    big = 1 << 40
    radius = (ctypes.c_double * 12)(*([0.75] * 12))
    records = ["lm" + k for k in "clnfsp"] + ["out" + k for k in "clnfsp"]

    def call(centers=g, labels=g, Q=8, N=10, poses=g, assoc=g, starts=None, n_sessions=0, session_base=2, node_base=160, rad=radius,
             n_labels=12, tau_z=0.75, L=20, cap=100, node=g, num=g, ws=g, wsb=big, **rec):
        r = [rec.get(k, g) for k in records]
        return lib.sgpr_landmark_update(centers, labels, Q, N, poses, assoc, starts, n_sessions, session_base, node_base, rad,
                                        n_labels, tau_z, *r[:6], L, cap, *r[6:], node, num, ws, wsb, None)

    def says(word):
        return b"sgpr_landmark_update" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ["centers", "labels", "poses", "assoc", "node", "num", "ws"] + records:
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(rad=None) == INVALID and says("h_radius")
    for name in ("Q", "N", "L", "cap", "node_base", "session_base"):
        assert call(**{name: -1}) == INVALID and says("max_landmarks" if name == "cap" else name) and says("negative"), name
    assert call(L=20, cap=19) == INVALID and says("max_landmarks") and says("below")
    # (the accepted neighbours are asked with Q == 0: a call that passes its checks with Q N > 0 would go to the device)
    assert call(session_base=64) == INVALID and says("session_base") and call(Q=0, session_base=63) == 0
    two, empty = (ctypes.c_int32 * 2)(0, 4), (ctypes.c_int32 * 2)(0, 0)
    assert call(starts=two, n_sessions=2, session_base=63) == INVALID and says("session_base")
    assert call(Q=0, starts=empty, n_sessions=2, session_base=63) == INVALID and says("session_base")
    assert call(Q=0, starts=empty, n_sessions=2, session_base=62) == 0
    for nl in (0, -1, 65):
        assert call(n_labels=nl) == INVALID and says("n_labels"), nl
    for bad in (-0.5, float("nan")):
        r = (ctypes.c_double * 12)(*([0.75] * 5 + [bad] + [0.75] * 6))
        assert call(rad=r) == INVALID and says("radius of label 5")
        assert call(tau_z=bad) == INVALID and says("tau_z")
    # the session table of the Q scans: sgpr.h's rules
    assert call(starts=two, n_sessions=0) == INVALID and says("session")
    assert call(starts=None, n_sessions=2) == INVALID and says("session")
    assert call(starts=(ctypes.c_int32 * 2)(1, 4), n_sessions=2) == INVALID and says("start at 0")
    assert call(starts=(ctypes.c_int32 * 3)(0, 5, 4), n_sessions=3) == INVALID and says("decreasing")
    assert call(starts=(ctypes.c_int32 * 2)(0, 9), n_sessions=2) == INVALID and says("past")
    assert call(n_sessions=65, starts=two) == INVALID and says("sessions")
    # node indices and counts that leave int32
    assert call(Q=1 << 16, N=(1 << 14) + 1) == INVALID and says("int32")           # Q N > 2^30
    assert call(Q=0x7fffffff, N=0x7fffffff) == INVALID and says("int32")
    assert call(Q=1 << 15, N=1 << 15, node_base=(1 << 30)) == INVALID and says("node_base")   # node_base + Q N = 2^31
    assert call(Q=1 << 15, N=1 << 15, node_base=(1 << 30) - 1, wsb=0) == INVALID and says("workspace")
    need = lib.sgpr_landmark_update_workspace_bytes(8, 10, 20)
    assert need > 0 and call(wsb=need - 1) == INVALID and says("workspace") and call(wsb=0) == INVALID and says("workspace")
    # the records may be NULL where there are none
    null_out = {k: None for k in records[6:]}
    null_in = {k: None for k in records[:6]}
    assert call(L=0, cap=0, wsb=0, **null_out, **null_in) == INVALID and says("workspace")
    assert call(L=0, cap=5, wsb=0, **null_in) == INVALID and says("workspace")
    assert call(L=0, cap=5, **null_out) == INVALID and says("NULL")
    # Q == 0 or N == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    none = dict(centers=None, labels=None, poses=None, assoc=None, node=None, num=None, ws=None, wsb=0, **null_out, **null_in)
    assert call(Q=0) == 0 and call(N=0) == 0 and call(Q=0, **none) == 0 and call(N=0, **none) == 0
    assert call(Q=0, cap=3) == INVALID and call(N=0, session_base=70) == INVALID and call(Q=0, L=-1) == INVALID
    assert call(Q=0, rad=None) == INVALID and call(N=0, n_labels=0) == INVALID and call(N=0, node_base=-2) == INVALID


def test_workspace_formula():
    from sg_pr_amd import landmarks
    for Q, N, L in ((1, 1, 0), (1, 1, 1), (2, 64, 11), (3, 100, 40), (5, 256, 300), (5, 257, 300), (7, 100, 1100), (300, 100, 513),
                    (4541, 100, 60000), (0, 100, 5), (7, 0, 5), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1 << 15, 1 << 15, 1),
                    (1 << 16, (1 << 14) + 1, 1), (0x7fffffff, 1, 7)):
        assert landmarks.update_workspace_bytes(Q, N, L) == ref.workspace_bytes(Q, N, L), (Q, N, L)
    # sgpr_landmark_map's workspace for the nodes, two int32 per node, two counter blocks; per landmark 24 + 8 + 8 + 4 + 24
    assert ref.workspace_bytes(1, 1, 0) == lref.workspace_bytes(1, 1) + 2 * 256 + 2 * 256
    assert ref.workspace_bytes(3, 100, 64) - ref.workspace_bytes(3, 100, 0) == 64 * 68 and ref.workspace_bytes(9, 9, 7) % 256 == 0


# ------------------------------------------------------------------ the rules, on hand-made cases
def test_one_observation_moves_centre_count_sessions_and_spread():
    lm = lm_of([(0.0, 0.0, 0.0), (9.0, 9.0, 0.0)], [0, 0], count=[1, 4], first=[3, 7], sessions=[1, 2], spread=[0.0, 0.125])
    out = one([(1.0, 0.0, 0.5), (3.0, 3.0, 0.0)], [0, 0], [0, -1], lm, session_base=5, node_base=100)
    assert out["num"].tolist() == [2, 2, 1, 0] and out["node_landmark"].tolist() == [[0, -1]]
    # centre (0.5, 0, 0.25); the old member lies 0.5 from it (the parallel-axis term), the new one too: spread 0.5
    assert out["center"][0].tolist() == [0.5, 0.0, 0.25] and out["count"].tolist() == [2, 4] and out["spread"][0] == 0.5
    assert out["sessions"].tolist() == [1 | (1 << 5), 2] and out["first"].tolist() == [3, 7] and out["label"].tolist() == [0, 0]
    assert same_record(out, lm, 1)
    # three members of spread s about c, one observation at c: the centre stays, Q = 3 s s
    lm = lm_of([(2.0, -1.0, 0.0)], [1], count=[3], spread=[0.5])
    out = one([(2.0, -1.0, 0.0)], [1], [0], lm)
    assert out["center"][0].tolist() == [2.0, -1.0, 0.0] and out["count"].tolist() == [4]
    assert out["spread"][0] == np.sqrt(np.float64(0.75 * 2 ** 24) / (4.0 * 2 ** 24))


def test_new_nodes_link_at_the_radius_and_at_tau_z():
    r = 0.75
    lm = lm_of([(50.0, 0.0, 0.0)], [0])
    out = one([(0.0, 0.0, 0.0), (0.75, 0.0, 0.0)], [0, 0], [-2, -2], lm, radius=r, node_base=40, session_base=3)
    assert out["num"].tolist() == [2, 2, 0, 2] and out["node_landmark"].tolist() == [[1, 1]]          # a distance exactly r
    assert out["count"].tolist() == [1, 2] and out["first"].tolist() == [0, 40] and out["sessions"].tolist() == [1, 8]
    assert out["center"][1].tolist() == [0.375, 0.0, 0.0] and out["spread"][1] == 0.375
    out = one([(0.0, 0.0, 0.0), (np.nextafter(F32(0.75), F32(1)), 0.0, 0.0)], [0, 0], [-2, -2], lm, radius=r, node_base=40)
    assert out["num"].tolist() == [3, 2, 0, 2] and out["node_landmark"].tolist() == [[1, 2]] and out["first"].tolist() == [0, 40, 41]
    z = F32(0.75)
    out = one([(0.0, 0.0, 0.0), (0.1, 0.0, z)], [0, 0], [-2, -2], lm, tau_z=0.75)                   # |dz| exactly tau_z
    assert out["node_landmark"].tolist() == [[1, 1]]
    out = one([(0.0, 0.0, 0.0), (0.1, 0.0, np.nextafter(z, F32(1)))], [0, 0], [-2, -2], lm, tau_z=0.75)
    assert out["node_landmark"].tolist() == [[1, 2]]
    # another label does not link; a new node ON an old landmark does not join it; old landmarks never merge
    lm = lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0])
    out = one([(0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.25, 0.0, 0.0)], [0, 1, 0], [-2, -2, 0], lm)
    assert out["node_landmark"].tolist() == [[2, 3, 0]] and out["num"].tolist() == [4, 3, 1, 2]
    assert out["count"].tolist() == [2, 1, 1, 1] and same_record(out, lm, 1)


def test_eligibility_boundaries():
    node = [(1.0, 0.0, 0.0)]
    # count 2^18 and 2^18 + 1
    for count, ok in ((262144, True), (262145, False), (0, False), (-3, False), (1, True)):
        lm = lm_of([(0.0, 0.0, 0.0)], [0], count=[count], spread=[0.25])
        out = one(node, [0], [0], lm)
        assert out["node_landmark"].tolist() == [[0 if ok else -1]] and out["num"].tolist() == [1, 1, int(ok), 0], count
        assert same_record(out, lm, 0) != ok and (not ok or out["count"][0] == count + 1)
    # |center n0| at 2^38 and just above, in every coordinate
    for k in range(3):
        for c, n0, ok in ((2.0 ** 37, 2, True), (np.nextafter(2.0 ** 37, np.inf), 2, False), (-2.0 ** 37, 2, True),
                          (2.0 ** 20, 262144, True), (np.nextafter(-2.0 ** 20, -np.inf), 262144, False)):
            centre = [0.0, 0.0, 0.0]
            centre[k] = c
            lm = lm_of([centre], [0], count=[n0])
            out = one(node, [0], [0], lm)
            assert out["node_landmark"].tolist() == [[0 if ok else -1]], (k, c)
            assert same_record(out, lm, 0) != ok
            if ok:                                               # the recovered sum is exact, and fits
                S = int(np.rint(c * n0 * 2.0 ** 24)) + int(np.rint(node[0][k] * 2.0 ** 24))
                assert out["center"][0, k] == np.float64(S) / (np.float64(n0 + 1) * 2.0 ** 24)
    # non-finite centres; spread 0, -0.0 (eligible), NaN, negative, infinite (not)
    for centre in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        lm = lm_of([centre], [0])
        out = one(node, [0], [0], lm)
        assert out["node_landmark"].tolist() == [[-1]] and same_record(out, lm, 0)
    for sp, ok in ((0.0, True), (-0.0, True), (np.nan, False), (-1e-300, False), (np.inf, False), (1e200, True)):
        lm = lm_of([(0.0, 0.0, 0.0)], [0], spread=[sp])
        out = one(node, [0], [0], lm)
        assert out["node_landmark"].tolist() == [[0 if ok else -1]] and same_record(out, lm, 0) != ok, sp
    assert one(node, [0], [0], lm_of([(0.0, 0.0, 0.0)], [0], spread=[-0.0]))["spread"][0] == 0.5
    assert one(node, [0], [0], lm_of([(0.0, 0.0, 0.0)], [0], spread=[1e200]))["spread"][0] == np.sqrt((2.0 ** 44 + 2.0 ** 22) / 2.0 ** 25)   # v is capped
    # labels: out of range, a radius-0 label, a mismatch
    radius = [0.75, 0.0, 0.75]
    lm = lm_of([(0.0, 0.0, 0.0)] * 4, [0, 1, 3, -1])
    out = one(node * 5, [0, 1, 2, 0, 0], [0, 1, 0, 2, 3], lm, radius=radius)
    assert out["node_landmark"].tolist() == [[0, -1, -1, -1, -1]] and out["num"].tolist() == [4, 4, 1, 0]
    assert out["count"].tolist() == [2, 1, 1, 1] and all(same_record(out, lm, i) for i in (1, 2, 3))


def test_association_values_outside_the_map_are_rejected():
    lm = lm_of([(0.0, 0.0, 0.0), (5.0, 0.0, 0.0)], [0, 0])
    nodes = [(0.1, 0.0, 0.0)] * 7
    out = one(nodes, [0] * 6 + [-1], [-3, 2, 2 ** 31 - 1, -1, 1, -2, 0], lm)
    assert out["node_landmark"].tolist() == [[-1, -1, -1, -1, 1, 2, -1]] and out["num"].tolist() == [3, 6, 1, 1]
    assert same_record(out, lm, 0) and out["count"].tolist() == [1, 2, 1]
    # a dead node (a pose that is not finite, a point past the limit) changes nothing whatever its association
    out = one(nodes[:2], [0, 0], [0, -2], lm, pose=(1.0, 0.0, np.inf, 0.0))
    assert out["node_landmark"].tolist() == [[-1, -1]] and out["num"].tolist() == [2, 0, 0, 0]
    assert all(same_record(out, lm, i) for i in (0, 1))


def test_session_bits_up_to_63():
    lm = lm_of([(0.0, 0.0, 0.0)], [0], sessions=[1 << 63 | 1])
    cen = np.zeros((3, 2, 3), F32)
    cen[:, 1, 0] = 20.0
    out = ref.update(cen, np.zeros((3, 2), np.int32), np.array([IDENT] * 3), np.array([[0, -2]] * 3, np.int32), lm,
                     starts=[0, 1, 1], session_base=61)
    # scans 0 | (none) | 1, 2: sessions 0, 2, 2 -> bits 61 and 63
    assert out["sessions"].tolist() == [(1 << 63) | (1 << 61) | 1, (1 << 63) | (1 << 61)] and out["count"].tolist() == [4, 3]
    out = ref.update(cen[:1], np.zeros((1, 2), np.int32), np.array([IDENT]), np.array([[0, -2]], np.int32), lm_of([(0.0, 0.0, 0.0)], [0]),
                     session_base=63)
    assert out["sessions"].tolist() == [(1 << 63) | 1, 1 << 63]


def test_max_landmarks_trims_the_records_and_nothing_else():
    c, l, p, a, lm = ref.make_case(3, 100, 40, 3)
    full = ref.update(c, l, p, a, lm, node_base=700, session_base=1)
    total = int(full["num"][0])
    assert total >= 43
    for cap in (40, 41, total, total + 9):
        out = ref.update(c, l, p, a, lm, node_base=700, session_base=1, max_landmarks=cap)
        assert out["num"].tolist() == full["num"].tolist() and out["node_landmark"].tobytes() == full["node_landmark"].tobytes()
        assert all(out[k].tobytes() == full[k][:cap].tobytes() and len(out[k]) == min(cap, total) for k in ref.RECORD)


def test_an_empty_map_is_the_batch_map_of_the_new_nodes():
    c, l, p, a, _ = ref.make_case(4, 90, 30, 5)
    empty = lm_of(np.zeros((0, 3)), [])
    a = np.where(a >= 0, -2, a)
    a[0, :7] = (0, 5, -3, -1, 2 ** 31 - 1, -2, -2)              # with L == 0 no id is inside the map
    out = ref.update(c, l, p, a, empty, starts=[0, 2], session_base=4, node_base=3600)
    want = lref.landmark_map(c, np.where(a == -2, l, -1), p, starts=[0, 2])
    assert out["num"].tolist() == [want["num"][0], (lref.landmark_map(c, l, p)["node_landmark"] >= 0).sum(), 0, want["num"][1]]
    assert out["node_landmark"].tobytes() == want["node_landmark"].tobytes() and want["num"][0] > 10
    assert out["first"].tolist() == (want["first"] + 3600).tolist() and out["sessions"].tolist() == (want["sessions"] << np.uint64(4)).tolist()
    assert all(out[k].tobytes() == want[k].tobytes() for k in ("center", "label", "count", "spread"))
    assert set(out["sessions"].tolist()) <= {16, 32, 48} and len(set(out["sessions"].tolist())) >= 2


def test_sums_wrap_and_distances_are_capped_as_defined():
    # an observation 2000 m from its landmark: d2 is capped at 2^20, and so is v
    lm = lm_of([(0.0, 0.0, 0.0)], [0], count=[1], spread=[0.0])
    out = one([(2000.0, 0.0, 0.0)], [0], [0], lm)
    assert out["center"][0, 0] == 1000.0 and out["spread"][0] == 1000.0          # 1000 m < the cap of 1024 m
    out = one([(4000.0, 0.0, 0.0)], [0], [0], lm)
    assert out["center"][0, 0] == 2000.0 and out["spread"][0] == 1024.0


# ------------------------------------------------------------------ the planted world
def associate(centers, labels, poses, lm, radius=0.75):
    return aref.align(centers, labels, poses, lm["center"], lm["label"], radius=radius, tau_z=0.75, iters=0)["node_landmark"]


def against_batch(up, batch, label):
    """the bars of DESIGN.md §32 on an updated map `up` against the batch map of the same nodes on the same poses; the
    `first` of every updated landmark is a flat index into the batch map's nodes -> the figures"""
    holder = batch["node_landmark"].reshape(-1)[up["first"]]
    assert (holder >= 0).all()
    same = batch["count"][holder] == up["count"]
    dc = np.abs(up["center"][same] - batch["center"][holder[same]]).max()
    ds = np.abs(up["spread"][same] - batch["spread"][holder[same]]).max()
    bits = (up["center"][same].tobytes() == batch["center"][holder[same]].tobytes())
    print("%s: landmarks %d, batch %d, same count %d (%.4f), centre off by %.3g m (bit-equal: %s), spread by %.3g m"
          % (label, up["count"].size, batch["count"].size, same.sum(), same.mean(), dc, bits, ds))
    assert same.mean() >= 0.95
    assert dc <= 1e-9 and ds <= 1e-6
    assert (up["sessions"][same] == batch["sessions"][holder[same]]).all()
    return same.mean(), dc, ds


@pytest.fixture(scope="module")
def worlds():
    from sg_pr_amd import synth
    out = {}
    for seed in range(4):
        w = synth.landmark_world(seed)
        N = w["labels"].shape[1]
        lm = lref.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=w["starts"][:2], radius=0.75, tau_z=0.75)
        rng = np.random.default_rng(500 + seed)
        start = synth._se2_compose(w["truth"][200:], synth._se2(rng.normal(0, 0.02, 100), rng.normal(0, 0.3, 100),
                                                                rng.normal(0, 0.3, 100)))
        cen, lab = w["centers"][200:], w["labels"][200:]
        use = (lm["count"] >= 3).astype(np.uint8)
        X = start
        for r in (2.0, 0.75):
            X = aref.align(cen, lab, X, lm["center"], lm["label"], lm_use=use, radius=r, iters=10, min_nodes=6)["poses"]
        out[seed] = {"w": w, "lm": lm, "N": N, "start": start, "aligned": X, "centers": cen, "labels": lab}
    return out


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_update_after_alignment_is_the_batch_map_but_for_bridges(worlds, seed):
    p = worlds[seed]
    w, lm, N = p["w"], p["lm"], p["N"]
    L = lm["count"].size
    X = p["aligned"]
    up = ref.update(p["centers"], p["labels"], X, associate(p["centers"], p["labels"], X, lm), lm, session_base=2, node_base=200 * N)
    batch = lref.landmark_map(w["centers"], w["labels"], np.concatenate((w["truth"][:200], X)), starts=w["starts"])
    node = up["node_landmark"]
    live = node != -1
    assert live.sum() == up["num"][1] == (lref.landmark_map(p["centers"], p["labels"], X)["node_landmark"] >= 0).sum()
    tr = w["transient_session"][np.where(w["node_id"][200:] >= 0, w["node_id"][200:], 0)]
    transient_new = (node[live & (tr == 2)] >= L).mean()
    permanent_old = (node[live & (tr == -1)] < L).mean()
    fresh = up["sessions"][L:]
    print("seed %d: landmarks %d -> %d, transient nodes new %.4f, permanent nodes on old landmarks %.4f, observed %d, new %d"
          % (seed, L, up["num"][0], transient_new, permanent_old, up["num"][2], up["num"][3]))
    against_batch(up, batch, "seed %d" % seed)
    assert transient_new >= 0.95 and permanent_old >= 0.98
    assert fresh.size > 0 and (fresh == np.uint64(1 << 2)).all()
    assert up["count"].astype(np.int64).sum() == lm["count"].astype(np.int64).sum() + up["num"][2] + up["num"][3]
    assert up["num"][2] + up["num"][3] == up["num"][1]           # every live node is explained or new: none is rejected here
    # from the unaligned start poses the map fills with duplicates: this is why the update comes after the alignment
    raw = ref.update(p["centers"], p["labels"], p["start"], associate(p["centers"], p["labels"], p["start"], lm), lm, session_base=2,
                     node_base=200 * N)
    raw_old = (raw["node_landmark"][(raw["node_landmark"] != -1) & (tr == -1)] < L).mean()
    print("seed %d: from the start poses, permanent nodes on old landmarks %.4f, landmarks %d" % (seed, raw_old, raw["num"][0]))
    assert raw_old < 0.8


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_chained_updates_at_the_true_poses(worlds, seed):
    w, N = worlds[seed]["w"], worlds[seed]["N"]
    lm = lref.landmark_map(w["centers"][:100], w["labels"][:100], w["truth"][:100])
    for d in (1, 2):
        sl = slice(100 * d, 100 * d + 100)
        args = (w["centers"][sl], w["labels"][sl], w["truth"][sl])
        lm = ref.update(*args, associate(*args, lm), lm, session_base=d, node_base=100 * d * N)
    batch = lref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"])
    against_batch(lm, batch, "seed %d chained" % seed)
    assert lm["count"].astype(np.int64).sum() == batch["num"][1]


# ------------------------------------------------------------------ mutants of the definition
def test_mutants_change_an_output():
    assert set(ref.MUTANTS) >= {"no_parallel_axis", "old_centre", "float_sum", "ids_high", "first_no_base", "session_no_base",
                                "recompute_unobserved", "new_links_obs"}
    c, l, p, a, lm = ref.make_case(6, 70, 200, 2)
    rng = np.random.default_rng(4)
    a = np.where((a >= 0) & (rng.random(a.shape) < 0.05), -2, a)   # known objects taken for new ones, beside their observations
    kw = dict(starts=[0, 3], session_base=3, node_base=5000)
    base = ref.update(c, l, p, a, lm, **kw)
    assert base["num"][2] > 250 and base["num"][3] > 20 and (np.bincount(a[a >= 0], minlength=200) == 0).sum() > 5
    changed = {}
    for m in ref.MUTANTS:
        out = ref.update(c, l, p, a, lm, mutant=m, **kw)
        changed[m] = sorted(k for k in base if out[k].tobytes() != base[k].tobytes())
    assert all(changed.values()), changed
    assert changed["no_parallel_axis"] == ["spread"] == changed["old_centre"] and "center" in changed["float_sum"]
    assert "node_landmark" in changed["ids_high"] and changed["first_no_base"] == ["first"]
    assert changed["session_no_base"] == ["sessions"] and "spread" in changed["recompute_unobserved"]
    assert "node_landmark" in changed["new_links_obs"] and "count" in changed["new_links_obs"]
    again = ref.update(c, l, p, a, lm, **kw)
    assert all(again[k].tobytes() == base[k].tobytes() for k in base)
    with pytest.raises(ValueError):
        ref.update(c, l, p, a, lm, mutant="nope")
