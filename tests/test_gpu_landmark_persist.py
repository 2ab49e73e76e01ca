"""The visibility tallies of a landmark map on the GPU (sgpr_landmark_persist, include/sgpr_landmark_persist.h, DESIGN.md
§33): expected, seen, keep, scan_stat, view and num equal to the NumPy definition (tests/landmark_persist_ref.py) byte for
byte - at the shapes where the launch geometry, the cell walk and the ownership rule change, with no landmark, no scan,
every node on one landmark, landmarks on both sides of the origin under an unbounded range, at every boundary of the
rules - then streams, dirty workspaces, repeatability, the Python layer and the planted world end to end.  Every output
and the workspace are pre-filled with 0xFF, and the outputs carry a margin that must stay 0xFF."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_persist_ref as ref  # noqa: E402
import landmark_ref as lref  # noqa: E402
import landmark_update_ref as uref  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
MARGIN = 5
IDENT = (1.0, 0.0, 0.0, 0.0)
DTYPES = {"expected": torch.int32, "seen": torch.int32, "keep": torch.uint8, "scan_stat": torch.int32, "view": torch.float64,
          "num": torch.int32}


def device_persist(centers, labels, poses, assoc, lm, radius=0.75, n_labels=None, max_range=50.0, margin=2.0, min_expected=5,
                   max_seen_ratio=0.3, stream=None, workspace=None, ws_fill=0xFF, out_fill=0xFF):
    """the C call with every output (and a margin behind it) full of the byte out_fill and the workspace full of ws_fill
    (a given workspace is used as it is) -> dict of host arrays"""
    from sg_pr_amd import engine, landmarks
    lib = landmarks.load_library()
    dev = torch.device("cuda", 0)
    lab = torch.as_tensor(np.ascontiguousarray(labels, np.int32)).to(dev)
    Q, N = lab.shape
    cen = torch.as_tensor(np.ascontiguousarray(centers, F32).reshape(Q, N, 3)).to(dev)
    X = torch.as_tensor(np.ascontiguousarray(poses, np.float64).reshape(Q, 4)).to(dev)
    asc = torch.as_tensor(np.ascontiguousarray(assoc, np.int32).reshape(Q * N)).to(dev)
    lm_c = torch.as_tensor(np.ascontiguousarray(lm["center"], np.float64).reshape(-1)).to(dev)
    lm_l = torch.as_tensor(np.ascontiguousarray(lm["label"], np.int32).reshape(-1)).to(dev)
    L = lm_l.numel()
    use = None if lm.get("use") is None else torch.as_tensor(np.ascontiguousarray(lm["use"], np.uint8)).to(dev)
    rad = np.atleast_1d(np.asarray(radius, np.float64))
    if rad.size == 1:
        rad = np.full(12 if n_labels is None else n_labels, rad[0])
    rad = np.ascontiguousarray(rad)
    sizes = {"expected": L, "seen": L, "keep": L, "scan_stat": 4 * Q, "view": Q, "num": 4}
    out = {k: torch.full(((sizes[k] + MARGIN) * t.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(t) for k, t in DTYPES.items()}
    need = landmarks.persist_workspace_bytes(Q, N, L)
    assert need == ref.workspace_bytes(Q, N, L)
    ws = torch.full((max(need, 1),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs and the fills were made on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_landmark_persist(
            p(cen), p(lab), Q, N, p(X), p(asc), p(lm_c) if L else None, p(lm_l) if L else None, p(use) if use is not None and L else None,
            L, rad.ctypes.data, rad.size, float(max_range), float(margin), int(min_expected), float(max_seen_ratio),
            p(out["expected"]), p(out["seen"]), p(out["keep"]), p(out["scan_stat"]), p(out["view"]), p(out["num"]), p(ws), need,
            engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, sizes


def check(centers, labels, poses, assoc, lm, **kw):
    """the outputs equal the reference byte for byte, nothing is written past any output -> the reference's dict"""
    extra = {k: kw.pop(k) for k in ("stream", "workspace", "ws_fill", "out_fill") if k in kw}
    out_fill = extra.get("out_fill", 0xFF)
    Q, N = np.asarray(labels).shape
    want = ref.persist(centers, labels, poses, assoc, lm, **kw)
    got, sizes = device_persist(centers, labels, poses, assoc, lm, **kw, **extra)
    if Q * N == 0:                                               # nothing is written
        assert all((v.view(np.uint8) == out_fill).all() for v in got.values())
        return want
    for name in ref.OUTPUTS:
        n = sizes[name]
        assert got[name][:n].tobytes() == np.ascontiguousarray(want[name]).tobytes(), (name, got[name][:n], want[name].reshape(-1))
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"
    return want


def lm_of(center, label, use=None):
    lm = {"center": np.array(center, np.float64).reshape(-1, 3), "label": np.array(label, np.int32)}
    if use is not None:
        lm["use"] = np.array(use, np.uint8)
    return lm


def scans(nodes, labels, assoc, lm, poses=None, **kw):
    q = len(nodes)
    return check(np.array(nodes, F32).reshape(q, -1, 3), np.array(labels, np.int32).reshape(q, -1),
                 np.array([IDENT] * q if poses is None else poses, np.float64), np.array(assoc, np.int32).reshape(q, -1), lm, **kw)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("Q,N,L", [(1, 1, 1), (3, 100, 40), (2, 130, 10), (70, 7, 500), (2, 1024, 3)])
def test_shapes(Q, N, L):
    """one scan, one node, one landmark; N no multiple of 64; more scans than a workgroup has waves and, with cells of 500 m
    or one cell for all, more landmarks in a coarse cell than a wave has lanes; 1024 nodes on three landmarks"""
    case = ref.make_case(Q, N, L, 1000 * Q + N)
    want = check(*case, max_range=10.0, margin=0.5, min_expected=2)
    check(*case, max_range=40.0, margin=2.0, min_expected=3, max_seen_ratio=0.5)
    check(*case, max_range=1000.0, margin=0.0, min_expected=2)
    check(*case, max_range=float("inf"), margin=0.5, min_expected=2)
    check(*case, max_range=6.0, margin=0.0, min_expected=0, max_seen_ratio=1.0, radius=[0.75, 0.0, 2.0], n_labels=3)
    no_mask = dict(case[4], use=None)
    check(*case[:4], no_mask, max_range=10.0, margin=0.5, min_expected=1)
    if L >= 40:
        assert want["seen"].sum() > 0 and (want["expected"] > want["seen"]).any() and want["num"][3] >= 1
    if L == 500:
        assert want["num"][0] > 5 and want["scan_stat"][:, 0].max() > 10


def test_every_node_of_a_scan_on_one_landmark():
    """ownership and contention: 1024 nodes of a scan observe one landmark and count once"""
    rng = np.random.default_rng(11)
    cen = np.concatenate((rng.normal(0.0, 0.2, size=(2, 1024, 2)), rng.uniform(-0.3, 0.3, size=(2, 1024, 1))), axis=2).astype(F32)
    cen[:, 500, 0] = 9.0
    lm = lm_of([(0.05, -0.02, 0.0), (3.0, 0.0, 0.0), (40.0, 0.0, 0.0)], [2, 2, 2])
    lab = np.full((2, 1024), 2, np.int32)
    assoc = np.zeros((2, 1024), np.int32)
    assoc[1, ::3] = 2                                            # a third of the second scan on a landmark beyond its view
    want = check(cen, lab, np.array([IDENT] * 2), assoc, lm, max_range=50.0, margin=2.0, min_expected=1)
    assert want["seen"].tolist() == [2, 0, 1] and want["expected"].tolist() == [2, 2, 1] and want["scan_stat"][:, :3].tolist() == [[2, 1, 1024], [3, 2, 1024]]
    assert want["keep"].tolist() == [1, 0, 1]


def test_cells_on_both_sides_of_the_origin_and_an_unbounded_range():
    c, l, p, a, lm = ref.make_case(9, 60, 300, 31, spread=30.0)
    assert (lm["center"][:, 0] < -20).any() and (lm["center"][:, 0] > 20).any() and (lm["center"][:, 1] < -20).any()
    want = check(c, l, p, a, lm, max_range=float("inf"), margin=1.0, min_expected=2)
    assert want["num"][3] >= 6 and want["view"].max() > 12 and want["num"][0] > 0
    for max_range in (3.0, 9.0, 25.0, 1e30):                     # cells of 1, 4, 12 m and one cell
        check(c, l, p, a, lm, max_range=max_range, margin=1.0, min_expected=2)
    # poses far from every landmark, and past the range of a cell coordinate
    far = p.copy()
    far[::2, 2] += 2.0 ** 36
    far[1::2, 3] = -1e300
    far[4, 2] = 1.7e308
    want = check(c, l, far, a, lm, max_range=float("inf"), margin=1.0, min_expected=0)
    assert (want["scan_stat"][:, 0] == want["scan_stat"][:, 1]).all()
    check(c, l, far, a, lm, max_range=20.0, margin=1.0, min_expected=0)
    # a live node 3e38 m from its sensor: a view range of 3e38 m, a pad and cell ends at the edge of the doubles
    big = float(F32(3e38))
    c[0, 0], l[0, 0], p[0] = (big, 0.0, 0.0), 0, (1.0, 0.0, 5.0 - big, 0.0)
    want = check(c, l, p, a, lm, max_range=float("inf"), margin=1.0, min_expected=0)
    assert want["view"][0] > 2.9e38 and want["scan_stat"][0, 2] == 1
    check(c, l, p, a, lm, max_range=20.0, margin=1.0, min_expected=0)


def test_no_landmark():
    c, l, p, a, lm = ref.make_case(6, 50, 0, 3)
    want = check(c, l, p, a, lm, max_range=8.0, margin=0.5)
    assert want["num"].tolist()[:3] == [0, 0, 0] and want["num"][3] == 0 and want["scan_stat"][:, 2].max() == 0
    c2 = ref.make_case(6, 50, 40, 3)
    want = check(*c2[:4], lm, max_range=8.0, margin=0.5)         # scans with live nodes, a map without landmarks
    assert want["num"].tolist()[:3] == [0, 0, 0] and want["num"][3] >= 3 and want["view"].max() > 0


def test_no_scan_and_no_slot_write_nothing():
    c, l, p, a, lm = ref.make_case(4, 10, 30, 6)
    check(c[:0], l[:0], p[:0], a[:0], lm)
    check(c[:, :0], l[:, :0], p, a[:, :0], lm)


def test_boundaries_of_the_rules():
    """the hand-made cases of tests/test_landmark_persist_host.py through the C call"""
    far = [(10.0, 0.0, 0.0)]
    kw = dict(max_range=50.0, margin=2.0, min_expected=1, max_seen_ratio=0.5)
    lm = lm_of([(8.0, 0.0, 0.0), (np.nextafter(8.0, 9.0), 0.0, 0.0), (0.0, -8.0, 5.0), (0.0, np.nextafter(-8.0, -9.0), 0.0), (4.8, -6.4, 0.0)], [0] * 5)
    want = scans([far], [[0]], [[-2]], lm, **kw)
    assert want["expected"].tolist() == [1, 0, 1, 0, 1]
    scans([far], [[0]], [[-2]], lm, poses=[(0.0, 1.0, 100.0, 0.0)], **kw)
    want = scans([far], [[0]], [[-2]], lm_of([(108.0, 0.0, 0.0), (np.nextafter(108.0, 109.0), 0.0, 0.0)], [0, 0]), poses=[(0.0, 1.0, 100.0, 0.0)], **kw)
    assert want["expected"].tolist() == [1, 0]
    scans([far], [[0]], [[-2]], lm_of([(4.0, 0.0, 0.0), (np.nextafter(4.0, 5.0), 0.0, 0.0)], [0, 0]), **dict(kw, max_range=6.0))
    scans([far], [[0]], [[-2]], lm, **dict(kw, max_range=float("inf")))
    scans([far + [(30.0, 0.0, 0.0)]], [[0, -1]], [[-2, -2]], lm, **kw)
    two = lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0])
    for margin in (10.0, 12.0, np.nextafter(10.0, 0.0)):
        scans([far], [[0]], [[-2]], two, **dict(kw, margin=margin))
    scans([far], [[0]], [[-2]], two, **dict(kw, max_range=0.0, margin=0.0))
    one = lm_of([(1.0, 0.0, 0.0)], [0])
    want = scans([far, far, far], [[-1], [0], [0]], [[0], [0], [0]], one, poses=[IDENT, (1.0, 0.0, np.nan, 0.0), (np.inf, 0.0, 0.0, 0.0)], **kw)
    assert want["scan_stat"].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1]]
    scans([far], [[0]], [[0]], one, poses=[(1.0, 0.0, 2.0 ** 37, 0.0)], **kw)
    pair = lm_of([(1.0, 0.0, 0.0), (3.0, 0.0, 0.0)], [0, 0])
    nodes = [(1.0, 0.1, 0.0), (10.0, 0.0, 0.0), (1.1, 0.0, 0.0), (0.9, 0.0, 0.0)]
    want = scans([nodes, nodes], [[0] * 4] * 2, [[0, -2, 0, 0], [-2, -2, 0, 0]], pair, **kw)
    assert want["seen"].tolist() == [2, 0] and want["expected"].tolist() == [2, 2]
    beyond = lm_of([(20.0, 0.0, 0.0), (1.0, 0.0, 0.0)], [0, 0])
    want = scans([far + [(1.0, 0.0, 0.0)]], [[0, 0]], [[0, 1]], beyond, **kw)
    assert want["expected"].tolist() == [1, 1] and want["seen"].tolist() == [1, 1]
    scans([far], [[0]], [[0]], beyond, **dict(kw, margin=11.0))
    odd = lm_of([(1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (3.0, 0.0, 0.0), (4.0, 0.0, 0.0), (5.0, 0.0, 0.0), (np.nan, 0.0, 0.0)],
                [0, 1, 0, 3, -1, 0], use=[1, 1, 0, 1, 1, 1])
    near = (1.0, 0.0, 0.0)
    want = scans([far + [near] * 11], [[0] * 11 + [-1]], [[-2, 1, 2, 3, 4, 5, -3, 6, 2 ** 31 - 1, -1, -2 ** 31, 0]], odd,
                 radius=[0.75, 0.75, 0.75, 0.0], **kw)
    assert want["seen"].tolist() == [0] * 6 and want["expected"].tolist() == [1, 1, 0, 0, 0, 0]
    see, miss = far + [(1.0, 0.0, 0.0)], far + [(5.0, 5.0, 0.0)]
    for seen, missed, more in ((0, 4, dict(min_expected=5)), (0, 5, dict(min_expected=5)), (2, 2, {}), (1, 3, {}), (3, 7, dict(max_seen_ratio=0.3)),
                               (3, 8, dict(max_seen_ratio=0.3)), (0, 6, dict(max_seen_ratio=0.0)), (6, 0, dict(max_seen_ratio=1.0)),
                               (5, 1, dict(max_seen_ratio=1.0))):
        scans([see] * seen + [miss] * missed, [[0, 0]] * (seen + missed), [[-2, 0]] * seen + [[-2, -2]] * missed, one, **dict(kw, **more))


# ------------------------------------------------------------------ streams, workspaces, repeatability
def test_a_stream_of_its_own_and_a_workspace_used_twice():
    case = ref.make_case(7, 100, 1100, 6)
    kw = dict(max_range=20.0, margin=1.0, min_expected=2)
    check(*case, stream=torch.cuda.Stream(), **kw)
    ws = torch.full((ref.workspace_bytes(7, 100, 1100),), 0xFF, dtype=torch.uint8, device="cuda")
    check(*case, workspace=ws, **kw)
    check(*case, workspace=ws, **kw)                             # dirty with the first call's state
    check(*ref.make_case(7, 100, 1100, 7), workspace=ws, **kw)


def test_two_calls_give_equal_bytes():
    case = ref.make_case(70, 7, 500, 9)
    kw = dict(max_range=15.0, margin=0.5, min_expected=2)
    a, _ = device_persist(*case, **kw)
    b, _ = device_persist(*case, **kw)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


# ------------------------------------------------------------------ the Python layer
def test_python_layer():
    from sg_pr_amd import landmarks
    c, l, p, a, lm = ref.make_case(12, 70, 200, 2)
    kw = dict(max_range=20.0, margin=1.0, min_expected=2, max_seen_ratio=0.5)
    want = ref.persist(c, l, p, a, lm, **kw)
    dev_lm = {"center": torch.as_tensor(lm["center"]).cuda(), "label": torch.as_tensor(lm["label"]).cuda()}
    raw = landmarks.persist_async(c, l, p, a, dev_lm, use=lm["use"], **kw)
    for k in ref.OUTPUTS:
        assert raw[k].is_cuda and raw[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    got = landmarks.persist(c, l, p, a, dev_lm, use=lm["use"], **kw)
    assert got["keep"].dtype == torch.bool and got["keep"].cpu().numpy().tolist() == (want["keep"] != 0).tolist()
    for k, col in (("scan_expected", 0), ("scan_seen", 1), ("scan_live", 2), ("flags", 3)):
        assert got[k].tolist() == want["scan_stat"][:, col].tolist(), k
    assert got["view"].tobytes() == want["view"].tobytes() and got["num"].tolist() == want["num"].tolist()
    # prior tallies are added in, the decision stays this call's
    prior = (np.arange(150, dtype=np.int32), np.arange(150, dtype=np.int32) // 2)
    life = landmarks.persist(c, l, p, a, dev_lm, use=lm["use"], prior=prior, **kw)
    assert life["expected"][:150].cpu().numpy().tolist() == (want["expected"][:150] + prior[0]).tolist()
    assert life["seen"].cpu().numpy().tolist() == (want["seen"] + np.pad(prior[1], (0, 50))).tolist()
    assert life["expected"][150:].cpu().numpy().tolist() == want["expected"][150:].tolist() and torch.equal(life["keep"], got["keep"])
    # select ANDs the mask, and is what it was without one
    rec = {"count": torch.arange(200, dtype=torch.int32).cuda() % 5, "sessions": torch.ones(200, dtype=torch.int64).cuda()}
    plain = landmarks.select(rec, min_count=3)
    assert torch.equal(landmarks.select(rec, min_count=3, keep=got["keep"]), plain & got["keep"]) and 0 < int((plain & ~got["keep"]).sum())
    assert torch.equal(landmarks.select(rec, min_count=3, keep=want["keep"]), plain & got["keep"])
    with pytest.raises(ValueError, match="keep"):
        landmarks.select(rec, keep=got["keep"][:5])
    short = torch.empty(landmarks.persist_workspace_bytes(12, 70, 200) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception, match="workspace"):
        landmarks.persist_async(c, l, p, a, dev_lm, workspace=short)
    with pytest.raises(Exception, match="max_seen_ratio"):
        landmarks.persist_async(c, l, p, a, dev_lm, max_seen_ratio=1.5)
    none = landmarks.persist(c[:0], l[:0], p[:0], a[:0], dev_lm)
    assert none["expected"].tolist() == [0] * 200 and bool(none["keep"].all()) and none["view"].shape == (0,) and none["num"].tolist() == [0] * 4


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_map_persistence_on_the_planted_world(model):
    """seed 0: drive 2 aligned to the map of drives 0 and 1, folded in (SG.update_map) and tallied on the updated map
    (SG.map_persistence) equals the reference pipeline; the mask feeds select and a second alignment"""
    from sg_pr_amd import landmarks, synth
    w = synth.landmark_world(0)
    N = w["labels"].shape[1]
    rng = np.random.default_rng(500)
    start = synth._se2_compose(w["truth"][200:], synth._se2(rng.normal(0, 0.02, 100), rng.normal(0, 0.3, 100), rng.normal(0, 0.3, 100)))
    cen, lab = w["centers"][200:], w["labels"][200:]
    lm = model.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], sessions=w["starts"][:2])
    X, _ = model.align_to_map(cen, lab, start, lm, keep=landmarks.select(lm, min_count=3))
    up = model.update_map(cen, lab, X, lm, 2, node_base=200 * N)
    got = model.map_persistence(cen, lab, X, up, node_landmark=up["node_landmark"])
    host = lref.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=w["starts"][:2])
    Z = X.cpu().numpy()
    assoc = aref.align(cen, lab, Z, host["center"], host["label"], radius=0.75, iters=0)["node_landmark"]
    hup = uref.update(cen, lab, Z, assoc, host, session_base=2, node_base=200 * N)
    want = ref.persist(cen, lab, Z, hup["node_landmark"], hup)
    assert got["expected"].cpu().numpy().tobytes() == want["expected"].tobytes() and got["seen"].cpu().numpy().tobytes() == want["seen"].tobytes()
    assert got["keep"].cpu().numpy().tolist() == (want["keep"] != 0).tolist() and got["view"].tobytes() == want["view"].tobytes()
    assert np.stack([got[k] for k in ("scan_expected", "scan_seen", "scan_live", "flags")], axis=1).tobytes() == want["scan_stat"].tobytes()
    assert got["num"].tolist() == want["num"].tolist() == [10, 108, 114, 100]
    # without node_landmark the nodes are associated with the updated map as update_map associates
    again = model.map_persistence(cen, lab, X, up)
    assoc2 = aref.align(cen, lab, Z, hup["center"], hup["label"], radius=0.75, iters=0)["node_landmark"]
    want2 = ref.persist(cen, lab, Z, assoc2, hup)
    assert again["seen"].cpu().numpy().tobytes() == want2["seen"].tobytes() and again["num"].tolist() == want2["num"].tolist()
    use = landmarks.select(up, min_count=3, keep=got["keep"])
    assert int(use.sum()) == int(landmarks.select(up, min_count=3).sum()) - 10
    Y, info = model.align_to_map(cen, lab, start, up, keep=use)
    truth = w["truth"][200:]
    Y = Y.cpu().numpy()
    assert np.median(np.hypot(Y[:, 2] - truth[:, 2], Y[:, 3] - truth[:, 3])) < 0.1 and info["accept"].all()


def test_place_db_retire_cli(model, tmp_path, ckpt_path, capsys):
    """--landmarks --sessions 3 --update --retire: <seq>_persist.npz holds the reference's tallies of the last session on the
    map <seq>_update.npz holds, and the printed line agrees with it; without --update the option is refused"""
    from sg_pr_amd import graph_store, place_db, synth
    centers, labels, _, poses = synth.world_sequence(90, 100, seed=4)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(90)])
    os.makedirs(tmp_path / "eva")
    seq.save(str(tmp_path / "eva" / "07_packed.npz"))
    cfg = tmp_path / "config.yml"
    cfg.write_text("""
common: {model: "%s", cuda: "0", batch_size: 128, p_thresh: 3, graph_pairs_dir: "%s", pair_list_dir: '%s'}
arch: {keep_node: 1, filters_1: 64, filters_2: 64, filters_3: 32, tensor_neurons: 16, bottle_neck_neurons: 16, K: 10}
train: {epochs: 500, train_sequences: ['00'], eval_sequences: ["08"], dropout: 0, learning_rate: 0.001,
        weight_decay: 0.0005, gpu: 0, logdir: "./logs_k10", node_num: 100}
eva_batch: {sequences: ["07"], output_path: "%s", show: False}
eva_pair: {pair_file: ["a.json", "b.json"]}
""" % (ckpt_path, tmp_path / "graphs", tmp_path, tmp_path / "eva"))
    place_db.main([str(cfg), "--k", "3", "--window", "14", "--landmarks", "--sessions", "3", "--update", "--retire", "--view-range", "30",
                   "--view-margin", "1.5", "--min-expected", "4", "--max-seen-ratio", "0.4"])
    lines = capsys.readouterr().out.splitlines()
    u = np.load(tmp_path / "eva" / "07_update.npz")
    z = np.load(tmp_path / "eva" / "07_persist.npz")
    lm = {"center": u["center"], "label": u["label"]}
    want = ref.persist(centers[60:], labels[60:], u["poses"], u["node_landmark"], lm, max_range=30.0, margin=1.5, min_expected=4,
                       max_seen_ratio=0.4)
    assert z["expected"].tobytes() == want["expected"].tobytes() and z["seen"].tobytes() == want["seen"].tobytes()
    assert z["keep"].tolist() == (want["keep"] != 0).tolist() and z["view"].tobytes() == want["view"].tobytes()
    assert np.stack([z[k] for k in ("scan_expected", "scan_seen", "scan_live", "flags")], axis=1).tolist() == want["scan_stat"].tolist()
    assert z["num"].tolist() == want["num"].tolist() and want["num"][1] > 20 and want["num"][3] == 30
    in_use = u["count"] >= 3
    assert int(z["in_use_before"]) == in_use.sum() and int(z["in_use_after"]) == (in_use & (want["keep"] != 0)).sum()
    assert float(z["max_range"]) == 30.0 and float(z["margin"]) == 1.5 and int(z["min_expected"]) == 4 and float(z["max_seen_ratio"]) == 0.4
    line = next(t for t in lines if "tallied on the updated map" in t)
    assert "landmarks in use %d -> %d, retired %d of %d judged" % (in_use.sum(), int(z["in_use_after"]), want["num"][0], want["num"][1]) in line
    assert "no occlusion model" in line and "%.4f" % float(z["scan_ratio_median"]) in line and 0.5 < float(z["scan_ratio_median"]) <= 1.0
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--landmarks", "--sessions", "3", "--retire"])
