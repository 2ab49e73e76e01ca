"""The incremental update of a landmark map on the GPU (sgpr_landmark_update, include/sgpr_landmark_update.h, DESIGN.md
§32): the six record arrays, node_landmark and num equal to the NumPy definition (tests/landmark_update_ref.py) to the
bit - at the shapes where the launch geometry and the cell table change, with no map, no observation, nothing but
observations of one landmark, at every boundary of the rules - then capacity, aliasing, streams, order-freedom, the
Python layer, the pipeline end to end and the command line.  Every output and the workspace are pre-filled with 0xFF,
and the outputs carry a margin that must stay 0xFF."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_ref as lref  # noqa: E402
import landmark_update_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
MARGIN = 5
IDENT = (1.0, 0.0, 0.0, 0.0)
DTYPES = {"center": torch.float64, "label": torch.int32, "count": torch.int32, "first": torch.int32, "sessions": torch.int64,
          "spread": torch.float64}
HOST = {"center": np.float64, "label": np.int32, "count": np.int32, "first": np.int32, "sessions": np.uint64, "spread": np.float64}


def device_update(centers, labels, poses, assoc, lm, starts=None, session_base=0, node_base=0, radius=0.75, tau_z=0.75,
                  n_labels=None, max_landmarks=None, stream=None, in_place=False, workspace=None, ws_fill=0xFF, out_fill=0xFF):
    """the C call with every output (and a margin behind it) full of the byte out_fill and the workspace full of ws_fill
    (a given workspace is used as it is) -> (dict of host arrays, cap)"""
    from sg_pr_amd import engine, landmarks
    lib = landmarks.load_library()
    dev = torch.device("cuda", 0)
    lab = torch.as_tensor(np.ascontiguousarray(labels, np.int32)).to(dev)
    Q, N = lab.shape
    cen = torch.as_tensor(np.ascontiguousarray(centers, F32).reshape(Q, N, 3)).to(dev)
    X = torch.as_tensor(np.ascontiguousarray(poses, np.float64).reshape(Q, 4)).to(dev)
    asc = torch.as_tensor(np.ascontiguousarray(assoc, np.int32).reshape(Q * N)).to(dev)
    old = {k: torch.as_tensor(np.ascontiguousarray(lm[k], HOST[k]).view(np.int64 if k == "sessions" else HOST[k]).reshape(-1)).to(dev)
           for k in ref.RECORD}
    L = old["label"].numel()
    cap = L + Q * N if max_landmarks is None else int(max_landmarks)
    rad = np.atleast_1d(np.asarray(radius, np.float64))
    if rad.size == 1:
        rad = np.full(12 if n_labels is None else n_labels, rad[0])
    rad = np.ascontiguousarray(rad)
    table = None if starts is None else np.ascontiguousarray(starts, np.int32)

    def dirty(n, dtype):
        return torch.full((n * dtype.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(dtype)

    out = {k: dirty((3 if k == "center" else 1) * (cap + MARGIN), DTYPES[k]) for k in ref.RECORD}
    out["node_landmark"] = dirty(Q * N + MARGIN, torch.int32)
    out["num"] = dirty(4 + MARGIN, torch.int32)
    if in_place:
        for k in ref.RECORD:
            out[k][:old[k].numel()] = old[k]
        out["node_landmark"][:Q * N] = asc
        old, asc = out, out["node_landmark"]
    need = landmarks.update_workspace_bytes(Q, N, L)
    assert need == ref.workspace_bytes(Q, N, L)
    ws = torch.full((max(need, 1),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs and the fills were made on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_landmark_update(
            p(cen), p(lab), Q, N, p(X), p(asc), None if table is None else table.ctypes.data, 0 if table is None else table.size,
            int(session_base), int(node_base), rad.ctypes.data, rad.size, float(tau_z),
            *[p(old[k]) if L or in_place else None for k in ref.RECORD], L, cap, *[p(out[k]) for k in ref.RECORD],
            p(out["node_landmark"]), p(out["num"]), p(ws), need, engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["sessions"] = got["sessions"].view(np.uint64)
    return got, cap


def same(got, want, cap, Q, N, out_fill=0xFF):
    """the outputs equal the reference to the bit (NaN as NaN: bytes), nothing written past the records found or past any
    output"""
    rows = min(int(want["num"][0]), cap)
    for name in ref.RECORD:
        w = 3 if name == "center" else 1
        assert len(want[name]) == rows
        assert got[name][:w * rows].tobytes() == np.ascontiguousarray(want[name], HOST[name]).tobytes(), \
            (name, got[name][:w * rows], want[name].reshape(-1))
        assert (got[name][w * rows:].view(np.uint8) == out_fill).all(), name + ": written past the records"
    for name, n in (("node_landmark", Q * N), ("num", 4)):
        assert got[name][:n].tobytes() == want[name].tobytes(), (name, got[name][:n], want[name].reshape(-1))
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"


def check(centers, labels, poses, assoc, lm, **kw):
    extra = {k: kw.pop(k) for k in ("stream", "in_place", "workspace", "ws_fill", "out_fill") if k in kw}
    out_fill = extra.get("out_fill", 0xFF)
    Q, N = np.asarray(labels).shape
    L = len(lm["label"])
    cap = kw.pop("max_landmarks", None)
    cap = L + Q * N if cap is None else cap
    want = ref.update(centers, labels, poses, assoc, lm, max_landmarks=cap, **kw)
    got, cap = device_update(centers, labels, poses, assoc, lm, max_landmarks=cap, **kw, **extra)
    if Q * N == 0:                                               # nothing is written
        assert all((v.view(np.uint8) == out_fill).all() for v in got.values())
        return want
    same(got, want, cap, Q, N, out_fill)
    return want


def lm_of(center, label, count=None, first=None, sessions=None, spread=None):
    n = len(label)
    return {"center": np.array(center, np.float64).reshape(-1, 3), "label": np.array(label, np.int32),
            "count": np.array([1] * n if count is None else count, np.int32),
            "first": np.array(list(range(n)) if first is None else first, np.int32),
            "sessions": np.array([1] * n if sessions is None else sessions, np.uint64),
            "spread": np.array([0.0] * n if spread is None else spread, np.float64)}


def one(nodes, labels, assoc, lm, pose=IDENT, **kw):
    return check(np.array([nodes], F32), np.array([labels], np.int32), np.array([pose], np.float64), np.array([assoc], np.int32),
                 lm, **kw)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("Q,N,L", [(1, 1, 1), (1, 64, 3), (3, 100, 40), (5, 256, 300), (5, 257, 300), (7, 100, 1100)])
def test_shapes(Q, N, L):
    """one block and one node; 256-thread blocks exact and ragged; 700 nodes: a cell table of 2048 slots"""
    case = ref.make_case(Q, N, L, 1000 * Q + N)
    want = check(*case, starts=None if Q < 3 else [0, 1, Q - 1], session_base=2, node_base=L * 7 + 3)
    if Q * N >= 64:
        assert want["num"][2] > Q * N // 2 and want["num"][3] >= 1 and want["num"][0] > L
    check(*case, radius=[0.75, 0.0, 2.0], tau_z=0.3, n_labels=3)


def test_no_map():
    c, l, p, a, _ = ref.make_case(4, 90, 30, 5)
    a = np.where(a >= 0, -2, a)
    a[0, :7] = (0, 5, -3, -1, 2 ** 31 - 1, -2, -2)
    want = check(c, l, p, a, lm_of(np.zeros((0, 3)), []), starts=[0, 2], session_base=4, node_base=3600)
    batch = lref.landmark_map(c, np.where(a == -2, l, -1), p, starts=[0, 2])
    assert want["center"].tobytes() == batch["center"].tobytes() and want["first"].tolist() == (batch["first"] + 3600).tolist()
    check(c, l, p, a, lm_of(np.zeros((0, 3)), []), max_landmarks=0)
    check(c, l, p, a, lm_of(np.zeros((0, 3)), []), max_landmarks=3, in_place=True)


def test_no_slots_and_no_scans():
    c, l, p, a, lm = ref.make_case(4, 10, 30, 6)
    check(c[:, :0], l[:, :0], p, a[:, :0], lm)
    check(c[:0], l[:0], p[:0], a[:0], lm)


def test_all_nodes_new():
    c, l, p, a, lm = ref.make_case(5, 130, 60, 8)
    want = check(c, l, p, np.full_like(a, -2), lm, session_base=1, node_base=9000)
    assert want["num"][2] == 0 and want["num"][3] == want["num"][1] > 500
    assert all(want[k][:60].tobytes() == np.ascontiguousarray(lm[k]).tobytes() for k in ref.RECORD)


def test_all_nodes_on_one_landmark():
    """the contention case: 1024 atomics on one set of accumulators, the same bits"""
    rng = np.random.default_rng(11)
    cen = np.concatenate((rng.normal(0.0, 0.2, size=(8, 128, 2)), rng.uniform(-0.3, 0.3, size=(8, 128, 1))), axis=2).astype(F32)
    lm = lm_of([(0.05, -0.02, 0.0)], [2], count=[37], first=[5], sessions=[3], spread=[0.21])
    want = check(cen, np.full((8, 128), 2, np.int32), np.array([IDENT] * 8), np.zeros((8, 128), np.int32), lm,
                 starts=[0, 4], session_base=2)
    assert want["count"].tolist() == [37 + 1024] and want["sessions"].tolist() == [15] and want["num"].tolist() == [1, 1024, 1024, 0]


def test_no_observation_at_all():
    c, l, p, a, lm = ref.make_case(5, 130, 300, 9)
    lm["spread"][:4] = (np.nan, -1.0, -0.0, np.inf)
    lm["center"][5, 1] = np.nan
    lm["center"].view(np.uint64)[6, 0] = 0xfff8000000abcdef    # payloads are copied
    for assoc in (np.where(a >= 0, -1, a), np.where(a >= 0, 300, a), np.full_like(a, -7)):
        want = check(c, l, p, assoc, lm)
        assert want["num"][2] == 0 and all(want[k][:300].tobytes() == np.ascontiguousarray(lm[k]).tobytes() for k in ref.RECORD)


# ------------------------------------------------------------------ the rules
def test_boundaries_of_the_rules():
    """the hand-made cases of tests/test_landmark_update_host.py through the C call"""
    node = [(1.0, 0.0, 0.0)]
    z = F32(0.75)
    lm = lm_of([(50.0, 0.0, 0.0)], [0])
    for far, dz in ((0.75, 0.0), (np.nextafter(z, F32(1)), 0.0), (0.1, z), (0.1, np.nextafter(z, F32(1)))):
        one([(0.0, 0.0, 0.0), (far, 0.0, dz)], [0, 0], [-2, -2], lm, radius=0.75, tau_z=0.75, node_base=40, session_base=3)
    for count in (262144, 262145, 0, -3, 1):
        want = one(node, [0], [0], lm_of([(0.0, 0.0, 0.0)], [0], count=[count], spread=[0.25]))
        assert want["num"][2] == (1 <= count <= 262144)
    for k in range(3):
        for c, n0 in ((2.0 ** 37, 2), (np.nextafter(2.0 ** 37, np.inf), 2), (-2.0 ** 37, 2), (2.0 ** 20, 262144),
                      (np.nextafter(-2.0 ** 20, -np.inf), 262144), (np.nan, 1), (-np.inf, 1)):
            centre = [0.0, 0.0, 0.0]
            centre[k] = c
            one(node, [0], [0], lm_of([centre], [0], count=[n0]))
    for sp in (0.0, -0.0, np.nan, -1e-300, np.inf, 1e200, 0.3):
        one(node, [0], [0], lm_of([(0.0, 0.0, 0.0)], [0], spread=[sp]))
    lm4 = lm_of([(0.0, 0.0, 0.0)] * 4, [0, 1, 3, -1])
    one(node * 5, [0, 1, 2, 0, 0], [0, 1, 0, 2, 3], lm4, radius=[0.75, 0.0, 0.75])
    lm2 = lm_of([(0.0, 0.0, 0.0), (5.0, 0.0, 0.0)], [0, 0])
    want = one([(0.1, 0.0, 0.0)] * 7, [0] * 6 + [-1], [-3, 2, 2 ** 31 - 1, -1, 1, -2, 0], lm2)
    assert want["node_landmark"].tolist() == [[-1, -1, -1, -1, 1, 2, -1]]
    one([(0.1, 0.0, 0.0)] * 2, [0, 0], [0, -2], lm2, pose=(1.0, 0.0, np.inf, 0.0))
    one([(0.1, 0.0, 0.0)] * 2, [0, 0], [0, -2], lm2, pose=(1.0, 0.0, np.nextafter(2.0 ** 37, np.inf), 0.0))
    one([(2000.0, 0.0, 0.0)], [0], [0], lm_of([(0.0, 0.0, 0.0)], [0]))
    want = one([(4000.0, 0.0, 0.0)], [0], [0], lm_of([(0.0, 0.0, 0.0)], [0]))
    assert want["spread"][0] == 1024.0
    # session bits up to 63
    cen = np.zeros((3, 2, 3), F32)
    cen[:, 1, 0] = 20.0
    want = check(cen, np.zeros((3, 2), np.int32), np.array([IDENT] * 3), np.array([[0, -2]] * 3, np.int32),
                 lm_of([(0.0, 0.0, 0.0)], [0], sessions=[1 << 63 | 1]), starts=[0, 1, 1], session_base=61)
    assert want["sessions"].tolist() == [(1 << 63) | (1 << 61) | 1, (1 << 63) | (1 << 61)]
    check(cen[:1], np.zeros((1, 2), np.int32), np.array([IDENT]), np.array([[0, -2]], np.int32), lm_of([(0.0, 0.0, 0.0)], [0]),
          session_base=63)


def test_capacity():
    """max_landmarks == L with new landmarks present - only d_num and the node ids tell of them -, L + 1, exact, ample"""
    c, l, p, a, lm = ref.make_case(3, 100, 40, 3)
    total = int(ref.update(c, l, p, a, lm)["num"][0])
    assert total >= 43
    for cap in (40, 41, total, total + 9):
        want = check(c, l, p, a, lm, node_base=700, session_base=1, max_landmarks=cap)
        assert want["num"][0] == total and want["node_landmark"].max() == total - 1 and len(want["label"]) == min(cap, total)


# ------------------------------------------------------------------ aliasing, streams, workspaces, order
@pytest.mark.parametrize("Q,N,L", [(3, 100, 40), (7, 100, 1100)])
def test_in_place(Q, N, L):
    case = ref.make_case(Q, N, L, 21)
    want = check(*case, session_base=2, node_base=123456, in_place=True)
    assert want["num"][2] > 100 and want["num"][0] > L
    check(*case, session_base=2, node_base=123456, in_place=True, max_landmarks=L)


def test_a_stream_of_its_own_and_a_workspace_used_twice():
    case = ref.make_case(7, 100, 1100, 6)
    check(*case, session_base=2, stream=torch.cuda.Stream())
    need = ref.workspace_bytes(7, 100, 1100)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    check(*case, session_base=2, workspace=ws)
    check(*case, session_base=2, workspace=ws)                   # dirty with the first call's state
    other = ref.make_case(7, 100, 1100, 7)
    check(*other, session_base=1, workspace=ws)


def test_scan_order_decides_nothing_but_the_numbering():
    c, l, p, a, lm = ref.make_case(7, 100, 300, 5)
    L = 300
    x = check(c, l, p, a, lm, node_base=4000)
    perm = np.random.default_rng(9).permutation(7)
    y = check(c[perm], l[perm], p[perm], a[perm], lm, node_base=4000)
    assert all(x[k][:L].tobytes() == y[k][:L].tobytes() for k in ref.RECORD)
    old_x, old_y = x["node_landmark"][perm], y["node_landmark"]
    assert (np.where(old_x < L, old_x, L) == np.where(old_y < L, old_y, L)).all() and x["num"].tolist() == y["num"].tolist()

    def fresh(o):
        return sorted((o["center"][i].tobytes(), int(o["label"][i]), int(o["count"][i]), int(o["sessions"][i]), o["spread"][i].tobytes())
                      for i in range(L, int(o["num"][0])))
    assert fresh(x) == fresh(y) and len(fresh(x)) > 5
    assert sorted(y["first"][L:].tolist()) == y["first"][L:].tolist()       # numbered by the lowest flat index


# ------------------------------------------------------------------ the Python layer
def test_python_layer():
    from sg_pr_amd import landmarks
    c, l, p, a, lm = ref.make_case(5, 130, 300, 4)
    want = ref.update(c, l, p, a, lm, starts=[0, 2], session_base=2, node_base=700)
    dev_lm = {k: torch.as_tensor(np.ascontiguousarray(lm[k]).view(np.int64) if k == "sessions" else lm[k]).cuda() for k in ref.RECORD}
    got = landmarks.update(c, l, p, a, dev_lm, starts=[0, 2], session_base=2, node_base=700)
    for k in ref.RECORD + ("node_landmark",):
        assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert [got[k] for k in ("num_landmarks", "live_nodes", "observed", "new_nodes")] == want["num"].tolist()
    assert dev_lm["count"].cpu().numpy().tobytes() == lm["count"].tobytes()      # the input map is left as it is
    # a capacity that is too small is repaired by a second call; host arrays are taken too
    got = landmarks.update(c, l, p, a, lm, starts=[0, 2], session_base=2, node_base=700, max_landmarks=300)
    assert got["num_landmarks"] == want["num"][0] and got["spread"].cpu().numpy().tobytes() == want["spread"].tobytes()
    raw = landmarks.update_async(c, l, p, a, dev_lm, max_landmarks=300)
    assert raw["num"].tolist()[0] > 300 and raw["label"].shape[0] == 300
    short = torch.empty(landmarks.update_workspace_bytes(5, 130, 300) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception, match="workspace"):
        landmarks.update_async(c, l, p, a, dev_lm, workspace=short)
    none = landmarks.update(c[:0], l[:0], p[:0], a[:0], dev_lm)
    assert none["num_landmarks"] == 300 and none["center"].cpu().numpy().tobytes() == lm["center"].tobytes()
    assert none["node_landmark"].shape == (0, 130) and none["observed"] == 0
    # an update feeds select, the next update and virtual scans
    keep = landmarks.select(got, min_count=3)
    assert keep.shape[0] == got["num_landmarks"] and 0 < int(keep.sum()) < keep.shape[0]
    again = landmarks.update(c, l, p, got["node_landmark"], got, session_base=3, node_base=2000)
    want2 = ref.update(c, l, p, want["node_landmark"], want, session_base=3, node_base=2000)
    assert again["count"].cpu().numpy().tobytes() == want2["count"].tobytes() and again["new_nodes"] == 0
    X, info = landmarks.refine(c, l, p, got, use=keep, iters=1, min_nodes=2)     # (its node_landmark is these scans')
    assert X.shape == (5, 4) and info["landmarks"] > 0
    vc, vl = landmarks.virtual_scans(got, p[:2], keep=keep)
    assert vc.shape == (2, 100, 3) and (vl >= 0).any()


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


def test_update_map_after_align_to_map(model):
    """seed 0 of the planted world: drive 2 aligned to the map of drives 0 and 1 (SG.align_to_map) and folded in
    (SG.update_map) equals the reference pipeline; the result feeds select and a second alignment"""
    from sg_pr_amd import landmarks, synth
    w = synth.landmark_world(0)
    N = w["labels"].shape[1]
    rng = np.random.default_rng(500)
    start = synth._se2_compose(w["truth"][200:], synth._se2(rng.normal(0, 0.02, 100), rng.normal(0, 0.3, 100), rng.normal(0, 0.3, 100)))
    cen, lab = w["centers"][200:], w["labels"][200:]
    lm = model.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], sessions=w["starts"][:2])
    keep = landmarks.select(lm, min_count=3)
    X, _ = model.align_to_map(cen, lab, start, lm, keep=keep)
    up = model.update_map(cen, lab, X, lm, 2)
    host = lref.landmark_map(w["centers"][:200], w["labels"][:200], w["truth"][:200], starts=w["starts"][:2])
    Z = X.cpu().numpy()
    assoc = aref.align(cen, lab, Z, host["center"], host["label"], radius=0.75, iters=0)["node_landmark"]
    base = (int(host["first"].max()) + N) // N * N             # the default: past the scan of the largest `first`
    want = ref.update(cen, lab, Z, assoc, host, session_base=2, node_base=base)
    assert base % N == 0 and host["first"].max() < base <= 200 * N and want["first"][len(host["first"]):].min() >= base
    for k in ref.RECORD + ("node_landmark",):
        assert up[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert [up[k] for k in ("num_landmarks", "live_nodes", "observed", "new_nodes")] == want["num"].tolist() == [114, 3898, 3673, 225]
    keep2 = landmarks.select(up, min_count=3)
    assert int(keep2.sum()) >= int(keep.sum()) and (up["sessions"][lm["num_landmarks"]:] == 4).all()
    Y, info = model.align_to_map(cen, lab, start, up, keep=keep2)
    truth = w["truth"][200:]
    Y = Y.cpu().numpy()
    assert np.median(np.hypot(Y[:, 2] - truth[:, 2], Y[:, 3] - truth[:, 3])) < 0.1 and info["accept"].all()


def test_place_db_update_cli(model, tmp_path, ckpt_path, capsys):
    """--landmarks --sessions 3 --update: the file holds the reference's pipeline on the sequence's own poses, num agrees
    with its arrays"""
    from sg_pr_amd import graph_store, metrics, place_db, synth
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
    place_db.main([str(cfg), "--k", "3", "--window", "14", "--landmarks", "--sessions", "3", "--update", "--align-radii", "1.5,0.75",
                   "--align-iters", "4"])
    lines = capsys.readouterr().out.splitlines()
    own = metrics.planar_odometry(poses)
    m = lref.landmark_map(centers[:60], labels[:60], own[:60], starts=[0, 30])
    Z = own[60:]
    for r in (1.5, 0.75):
        Z = aref.align(centers[60:], labels[60:], Z, m["center"], m["label"], radius=r, iters=4, min_nodes=6)["poses"]
    assoc = aref.align(centers[60:], labels[60:], Z, m["center"], m["label"], radius=0.75, iters=0)["node_landmark"]
    want = ref.update(centers[60:], labels[60:], Z, assoc, m, session_base=2, node_base=6000)
    z = np.load(tmp_path / "eva" / "07_update.npz")
    assert z["poses"].tobytes() == Z.tobytes() and z["start"].tobytes() == own[60:].tobytes()
    for k in ref.RECORD + ("node_landmark",):
        assert z[k].view(want[k].dtype).tobytes() == want[k].tobytes(), k
    num = z["num"].tolist()
    assert num == want["num"].tolist() and num[0] == len(z["count"]) == len(z["center"]) and int(z["landmarks_before"]) == len(m["count"])
    assert z["node_landmark"].max() < num[0] and (z["node_landmark"] >= 0).sum() == num[2] + num[3] <= num[1]
    assert z["count"].sum() == m["count"].sum() + num[2] + num[3] and int(z["session"]) == 2 and int(z["node_base"]) == 6000
    line = next(t for t in lines if "folded into the landmark map" in t)
    assert "landmarks %d -> %d (%d new)" % (len(m["count"]), num[0], num[0] - len(m["count"])) in line
    assert "observed nodes %d, new nodes %d" % (num[2], num[3]) in line and "%.4f" % float(z["same_count"]) in line
    batch = lref.landmark_map(centers, labels, np.concatenate((own[:60], Z)), starts=[0, 30, 60])
    same = batch["count"][batch["node_landmark"].reshape(-1)[want["first"]]] == want["count"]
    assert abs(float(z["same_count"]) - same.mean()) < 1e-12 and int(z["batch_landmarks"]) == batch["num"][0]
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--landmarks", "--update"])
