"""The landmark refinement (sgpr_landmark_refine, include/sgpr_landmark_refine.h) without a GPU: the C-ABI
surface of the fifth header and its argument checks, the NumPy definition (tests/landmark_refine_ref.py) on hand-made
cases and on synth.landmark_world after a pose-graph solve - the conditions that make the stage worth having - and
mutants of the definition that must each change an output."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_ref as lref  # noqa: E402
import landmark_refine_ref as ref  # noqa: E402
import posegraph_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
IDENT = (1.0, 0.0, 0.0, 0.0)
F32 = np.float32
SQUARE = [(1.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (-1.0, -1.0, 0.0), (1.0, -1.0, 0.0)]


def se2(yaw, x, y):
    return (math.cos(yaw), math.sin(yaw), x, y)


# ------------------------------------------------------------------ C-ABI surface
def test_fifth_header_parses_and_is_bound_with_the_parsed_types():
    from sg_pr_amd import _build, engine, landmarks, localize, posegraph
    text = open(os.path.join(REPO, "include", "sgpr_landmark_refine.h")).read()
    abi = _build.parse_header(text)
    assert [n for n, _, _ in abi.functions] == ["sgpr_landmark_refine_workspace_bytes", "sgpr_landmark_refine"] \
        == landmarks.REFINE_ABI_SYMBOLS
    assert abi.constants == {} and abi.errors == {}
    lib = landmarks.load_library()
    assert lib is engine.load_library()
    for name, restype, argtypes in abi.functions:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    (_, r0, a0), (_, r1, a1) = abi.functions
    assert r0 is ctypes.c_size_t and a0 == [ctypes.c_int] * 3
    assert r1 is ctypes.c_int and len(a1) == 16
    assert [a1[i] for i in (1, 2, 6, 8, 9)] == [ctypes.c_int] * 5 and a1[14] is ctypes.c_size_t
    assert all(a1[i] is ctypes.c_void_p for i in (0, 3, 4, 5, 7, 10, 11, 12, 13, 15))
    # the build lists, and the other four headers are what they were
    assert "sgpr_landmark_refine.hip" in _build.SOURCES
    assert any(h.endswith(os.path.join("include", "sgpr_landmark_refine.h")) for h in _build.HEADERS[1:-1])
    assert _build.HEADERS[0].endswith(os.path.join("include", "sgpr.h")) and _build.HEADERS[-1].endswith("sgpr_posegraph.h")
    assert len(_build.header_abi().functions) == 100 and _build.header_abi_version() == 11 == lib.sgpr_abi_version()
    assert not any("refine" in n for n in engine.ABI_SYMBOLS)
    assert landmarks.ABI_SYMBOLS == ["sgpr_landmark_workspace_bytes", "sgpr_landmark_map"]
    assert len(posegraph.ABI_SYMBOLS) == 2 and localize.ABI_SYMBOLS == ["sgpr_localize_scans"]


def test_argument_errors_never_touch_the_device():
    """Every documented argument error comes back with wild device pointers: had the device been touched, the call would
    have failed with SGPR_E_HIP (no GPU) or crashed."""
    from sg_pr_amd import landmarks
    lib = landmarks.load_library()
    g = ctypes.c_void_p(0xdead0000)          # never dereferenced
    big = 1 << 40

    def call(centers=g, G=8, N=10, poses=g, node=g, use=g, L=20, fixed=g, iters=3, min_nodes=6, out=g, cost=g, info=g, ws=g,
             wsb=big):
        return lib.sgpr_landmark_refine(centers, G, N, poses, node, use, L, fixed, iters, min_nodes, out, cost, info, ws, wsb,
                                        None)

    def says(word):
        return b"sgpr_landmark_refine" in lib.sgpr_last_error() and word.encode() in lib.sgpr_last_error()

    for name in ("centers", "poses", "node", "use", "out", "cost", "info", "ws"):
        assert call(**{name: None}) == INVALID and says("NULL"), name
    assert call(G=-1) == INVALID and says("G ") and call(N=-1) == INVALID and says("N ")
    assert call(L=-1) == INVALID and says("L ") and call(iters=-1) == INVALID and says("iters")
    for mn in (1, 0, -5):
        assert call(min_nodes=mn) == INVALID and says("min_nodes"), mn
    assert call(G=1 << 16, N=1 << 15) == INVALID and says("int32")
    assert call(G=0x7fffffff, N=0x7fffffff) == INVALID and says("int32")
    need = lib.sgpr_landmark_refine_workspace_bytes(8, 10, 20)
    assert call(wsb=need - 1) == INVALID and says("workspace") and call(wsb=0) == INVALID and says("workspace")
    # G == 0 or N == 0 succeeds without a launch, whatever the pointers are - but not with a bad argument beside it
    none = dict(centers=None, poses=None, node=None, use=None, fixed=None, out=None, cost=None, info=None, ws=None, wsb=0)
    assert call(G=0) == 0 and call(N=0) == 0 and call(G=0, **none) == 0 and call(N=0, **none) == 0
    assert call(G=0, min_nodes=1) == INVALID and call(N=0, iters=-2) == INVALID and call(G=0, L=-1) == INVALID


def test_workspace_formula():
    from sg_pr_amd import landmarks
    for G, N, L in ((1, 1, 0), (1, 1, 1), (2, 64, 11), (300, 100, 3200), (4541, 100, 60000), (5 * 4541, 100, 300000),
                    (0, 100, 5), (7, 0, 5), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1 << 16, 1 << 15, 1), (0x7fffffff, 1, 7)):
        assert landmarks.refine_workspace_bytes(G, N, L) == ref.workspace_bytes(G, N, L), (G, N, L)
    # two accumulator sets of three 64-bit words per landmark, two pose arrays, the scalars
    assert ref.workspace_bytes(300, 100, 3200) == 2 * 3 * 8 * 3200 + 256 + 2 * (32 * 300 + 128)      # (9600 -> 9728)
    assert ref.workspace_bytes(1, 1, 0) == 256 + 2 * 256 and ref.workspace_bytes(1, 1, 1) % 256 == 0


# ------------------------------------------------------------------ the rules, on hand-made cases
def two_squares(pose_b, **kw):
    """two scans that see the same square of four landmarks; scan 0 at the identity, scan 1 at pose_b"""
    centers = np.array([SQUARE, SQUARE], F32)
    ids = np.array([[0, 1, 2, 3], [0, 1, 2, 3]], np.int32)
    return ref.refine(centers, ids, np.array([IDENT, pose_b]), np.ones(4, np.uint8), min_nodes=2, **kw)


def test_one_iteration_moves_halfway_and_a_fixed_partner_is_converged_onto():
    yaw, tx, ty = 0.3, 0.5, -0.2
    out = two_squares(se2(yaw, tx, ty), iters=1)
    # the centres lie midway; both scans are fitted onto them: the pose halfway along the motion (the square is centred)
    half = np.array(se2(yaw / 2, tx / 2, ty / 2))
    assert np.abs(out["poses"] - half).max() < 1e-6
    d = np.array(SQUARE)[:, :2]
    moved = d @ np.array([[math.cos(yaw), math.sin(yaw)], [-math.sin(yaw), math.cos(yaw)]]) + (tx, ty)
    assert abs(out["cost"][0] - math.sqrt(np.mean(np.sum((moved - d) ** 2, axis=1)) / 4)) < 1e-6
    assert out["cost"][1] < 1e-6 and out["info"].tolist() == [8, 4, 2, 0]
    # scan 0 fixed: scan 1 halves its distance to it in every step
    out = two_squares(se2(yaw, tx, ty), iters=1, fixed=[1, 0])
    assert out["poses"][0].tolist() == list(IDENT) and np.abs(out["poses"][1] - half).max() < 1e-6
    assert out["info"].tolist() == [8, 4, 1, 0]
    out = two_squares(se2(yaw, tx, ty), iters=30, fixed=[1, 0])
    assert out["poses"][0].tolist() == list(IDENT) and np.abs(out["poses"][1] - IDENT).max() < 1e-6
    ratio = out["cost"][1:6] / out["cost"][:5]
    assert np.abs(ratio - 0.5).max() < 0.02 and out["cost"][-1] < 1e-6


def test_keep_rule():
    far = se2(0.3, 0.5, -0.2)
    centers = np.array([SQUARE, SQUARE], F32)
    ids = np.array([[0, 1, 2, 3], [0, 1, 2, -1]], np.int32)       # scan 1 has three used nodes
    X = np.array([IDENT, far])
    use = np.ones(4, np.uint8)
    out = ref.refine(centers, ids, X, use, iters=1, min_nodes=4)
    assert out["poses"][1].tobytes() == X[1].tobytes() and out["poses"][0].tobytes() != X[0].tobytes()
    assert out["info"].tolist() == [7, 4, 1, 1]
    out = ref.refine(centers, ids, X, use, iters=1, min_nodes=3)
    assert out["poses"][1].tobytes() != X[1].tobytes() and out["info"].tolist() == [7, 4, 2, 0]
    # all nodes of a scan coincident: p' is exactly 0, the moments vanish, h == 0
    same = np.array([SQUARE, [SQUARE[0]] * 4], F32)
    out = ref.refine(same, np.array([[0, 1, 2, 3]] * 2, np.int32), X, use, iters=2, min_nodes=2)
    assert out["poses"][1].tobytes() == X[1].tobytes() and out["info"][2:].tolist() == [1, 1]
    # a fixed scan keeps its bits, even bits no fit would produce
    odd = np.array([(0.6, 0.7, 0.1, 0.2), far])
    out = ref.refine(centers, np.array([[0, 1, 2, 3]] * 2, np.int32), odd, use, iters=3, min_nodes=2, fixed=[1, 0])
    assert out["poses"][0].tobytes() == odd[0].tobytes() and out["info"].tolist() == [8, 4, 1, 0]


def test_nothing_in_use_and_no_iterations():
    far = se2(0.3, 0.5, -0.2)
    X = np.array([IDENT, far])
    centers = np.array([SQUARE, SQUARE], F32)
    ids = np.array([[0, 1, 2, 3]] * 2, np.int32)
    out = ref.refine(centers, ids, X, np.zeros(4, np.uint8), iters=2, min_nodes=2)
    assert np.isnan(out["cost"]).all() and out["cost"].size == 3 and out["poses"].tobytes() == X.tobytes()
    assert out["info"].tolist() == [0, 0, 0, 2]
    assert out["cost"].view(np.uint64).tolist() == [0x7ff8000000000000] * 3
    # T == 0: the cost of the input, the input's bits
    out = ref.refine(centers, ids, X, np.ones(4, np.uint8), iters=0, min_nodes=2)
    assert out["cost"].size == 1 and out["cost"][0] > 0.1 and out["poses"].tobytes() == X.tobytes()
    assert out["info"].tolist() == [8, 4, 0, 0]
    # a mask over the landmarks: landmark 3 out, its nodes are not counted
    out = ref.refine(centers, ids, X, np.array([1, 1, 1, 0], np.uint8), iters=1, min_nodes=2)
    assert out["info"].tolist() == [6, 3, 2, 0]


def test_non_finite_poses_and_the_limit():
    centers = np.array([SQUARE] * 3, F32)
    ids = np.array([[0, 1, 2, 3]] * 3, np.int32)
    X = np.array([IDENT, se2(0.1, 0.2, 0.0), (np.nan, 0.0, 0.0, 0.0)])
    out = ref.refine(centers, ids, X, np.ones(4, np.uint8), iters=2, min_nodes=2)
    assert out["poses"][2].tobytes() == X[2].tobytes() and np.isfinite(out["poses"][:2]).all()
    assert out["info"].tolist() == [8, 4, 2, 1] and np.isfinite(out["cost"]).all()
    # a map point at 2^37 is used, one ulp past it is not
    zero = np.zeros((2, 1, 3), F32)
    edge = np.array([(1.0, 0.0, 2.0 ** 37, 0.0), (1.0, 0.0, np.nextafter(2.0 ** 37, np.inf), 0.0)])
    out = ref.refine(zero, np.zeros((2, 1), np.int32), edge, np.ones(1, np.uint8), iters=0, min_nodes=2)
    assert out["info"].tolist() == [1, 1, 0, 0] and out["cost"][0] == 0.0
    out = ref.refine(zero, np.zeros((2, 1), np.int32), edge[::-1], np.ones(1, np.uint8), iters=0, min_nodes=2)
    assert out["info"][0] == 1
    out = ref.refine(zero[:1], np.zeros((1, 1), np.int32), edge[1:], np.ones(1, np.uint8), iters=0, min_nodes=2)
    assert out["info"].tolist() == [0, 0, 0, 0] and np.isnan(out["cost"][0])


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
    many = rng.normal(size=(32, 130))
    assert (ref.scan_sum(many, np.ones((32, 130), bool)) != ref.scan_sum(many, np.ones((32, 130), bool), "sequential")).any()


# ------------------------------------------------------------------ the conditions, on the reference alone
@pytest.fixture(scope="module")
def runs():
    """seed -> the world, the pose graph's poses on closures with planted noise, two rounds of (landmark map, 10
    iterations) with the landmarks of count >= 2 and scan 0 fixed"""
    from sg_pr_amd import synth
    out = {}
    for seed in range(4):
        w = synth.landmark_world(seed)
        rng = np.random.default_rng(100 + seed)
        rows, cols = w["rows"].astype(np.int64), w["cols"].astype(np.int64)
        n = rows.size
        noise = synth._se2(rng.normal(0, 0.002, n), rng.normal(0, 0.04, n), rng.normal(0, 0.04, n))
        T = synth._se2_compose(noise, synth._se2_compose(synth._se2_inverse(w["truth"][cols]), w["truth"][rows]))
        X = posegraph_ref.optimize(w["odom"], rows, cols, T, starts=w["starts"])[0]
        fixed = np.zeros(X.shape[0], np.uint8)
        fixed[0] = 1
        Y, costs = X, []
        for _ in range(2):
            lm = lref.landmark_map(w["centers"], w["labels"], Y, starts=w["starts"])
            res = ref.refine(w["centers"], lm["node_landmark"], Y, (lm["count"] >= 2).astype(np.uint8), fixed=fixed, iters=10)
            Y = res["poses"]
            costs.append(res["cost"])
        out[seed] = {"w": w, "X": X, "Y": Y, "costs": costs, "info": res["info"]}
    return out


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_refinement_sharpens_the_map_and_the_trajectory(runs, seed):
    from sg_pr_amd import metrics
    r = runs[seed]
    w, X, Y = r["w"], r["X"], r["Y"]

    def sharp(poses):
        return metrics.map_sharpness(lref.landmark_map(w["centers"], w["labels"], poses, starts=w["starts"]))["sharpness"]

    tru, opt, got = sharp(w["truth"]), sharp(X), sharp(Y)
    e_opt, e_ref = metrics.trajectory_error(X, w["truth"]), metrics.trajectory_error(Y, w["truth"])
    print("seed %d: sharpness at truth %.4f, optimised %.4f, refined %.4f (%.3f x truth); trajectory error %.4f -> %.4f m "
          "(%.2f x); first round's cost %s" % (seed, tru, opt, got, got / tru, e_opt, e_ref, e_ref / e_opt,
                                                np.round(r["costs"][0], 4).tolist()))
    for cost in r["costs"]:
        assert (cost[1:] <= cost[:-1] * (1.0 + 1e-9)).all(), cost
    assert got <= 1.02 * tru
    assert e_ref <= 0.5 * e_opt
    assert Y[0].tobytes() == X[0].tobytes() and r["info"][2] == X.shape[0] - 1


# ------------------------------------------------------------------ mutants of the definition
def test_mutants_change_an_output():
    assert set(ref.MUTANTS) >= {"sequential", "fused_ar", "uncentred", "gauss_seidel", "float_centres"}
    rng = np.random.default_rng(2)
    G, N, L = 6, 70, 60
    pts = rng.uniform(-20.0, 20.0, size=(L, 2))
    ids = rng.integers(0, L, size=(G, N))
    yaw, t = rng.uniform(-3, 3, size=G), rng.uniform(-5, 5, size=(G, 2))
    d = pts[ids] + rng.normal(0, 0.1, size=(G, N, 2)) - t[:, None, :]
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    centers = np.stack((c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0], np.zeros((G, N))), axis=-1).astype(F32)
    yaw = yaw + rng.normal(0, 0.02, size=G)
    X = np.stack((np.cos(yaw), np.sin(yaw), t[:, 0] + rng.normal(0, 0.2, size=G), t[:, 1] + rng.normal(0, 0.2, size=G)), axis=1)
    args = (centers, ids.astype(np.int32), X, np.ones(L, np.uint8))
    base = ref.refine(*args, iters=2, min_nodes=2)
    assert base["info"].tolist() == [G * N, L, G, 0] and base["cost"][2] < base["cost"][0]
    changed = {}
    for m in ref.MUTANTS:
        out = ref.refine(*args, iters=2, min_nodes=2, mutant=m)
        changed[m] = any(out[k].tobytes() != base[k].tobytes() for k in base)
        # every mutant is a refinement all the same: it is the bits that tell them apart
        assert out["cost"][2] < out["cost"][0], m
        assert m == "uncentred" or np.abs(out["poses"] - base["poses"]).max() < 0.05, m
    assert all(changed.values()), changed
    again = ref.refine(*args, iters=2, min_nodes=2, mutant=None)
    assert all(again[k].tobytes() == base[k].tobytes() for k in base)
    with pytest.raises(ValueError):
        ref.refine(*args, mutant="nope")
