"""The record-level merge of landmark maps on the GPU (sgpr_landmark_merge, include/sgpr_landmark_merge.h):
the six record arrays, old_to_new and num equal to the NumPy definition (tests/landmark_merge_ref.py) to the bit - at the
sizes where the launch geometry and the cell table change, on every hand-made and mutant case of the reference, with and
without keep masks and poses, at every capacity, at the structural points of the kernels - then streams, the Python layer,
SG.register_maps + merge_maps and the command line.  Every output and the workspace are pre-filled with 0xFF, the outputs
carry a margin that must stay 0xFF, and the inputs must come back unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_merge_ref as ref  # noqa: E402
import landmark_persist_ref as pref  # noqa: E402
import landmark_ref as lref  # noqa: E402
import landmark_update_ref as uref  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 5
DTYPES = {"center": torch.float64, "label": torch.int32, "count": torch.int32, "first": torch.int32, "sessions": torch.int64,
          "spread": torch.float64}
HOST = {"center": np.float64, "label": np.int32, "count": np.int32, "first": np.int32, "sessions": np.uint64, "spread": np.float64}


def to_device(lm, dev):
    if lm is None:
        return None
    return {k: torch.as_tensor(np.ascontiguousarray(lm[k], HOST[k]).view(np.int64 if k == "sessions" else HOST[k]).reshape(-1)).to(dev)
            for k in ref.RECORD}


def launch(case, max_out=None, stream=None, workspace=None, ws_fill=0xFF, out_fill=0xFF):
    """the C call with every output (and a margin behind it) full of the byte out_fill and the workspace full of ws_fill
    (a given workspace is used as it is), asynchronous -> what finish needs"""
    from sg_pr_amd import engine, landmarks
    lib = landmarks.load_library()
    dev = torch.device("cuda", 0)
    kw = case["kw"]
    a, b = to_device(case["a"], dev), to_device(case["b"], dev)
    L_a, L_b = a["label"].numel(), 0 if b is None else b["label"].numel()
    T = L_a + L_b
    keeps = [None if kw.get(k) is None else torch.as_tensor(np.ascontiguousarray(kw[k], np.uint8)).to(dev) for k in ("keep_a", "keep_b")]
    cap = T if max_out is None else int(max_out)
    rad = np.atleast_1d(np.asarray(kw.get("radius", 0.75), np.float64))
    if rad.size == 1:
        rad = np.full(kw.get("n_labels") or 12, rad[0])
    rad = np.ascontiguousarray(rad)
    pose = None if kw.get("pose") is None else np.ascontiguousarray(kw["pose"], np.float64)

    def dirty(n, dtype):
        return torch.full((n * dtype.itemsize,), out_fill, dtype=torch.uint8, device=dev).view(dtype)

    out = {k: dirty((3 if k == "center" else 1) * (cap + MARGIN), DTYPES[k]) for k in ref.RECORD}
    out["old_to_new"] = dirty(T + MARGIN, torch.int32)
    out["num"] = dirty(4 + MARGIN, torch.int32)
    need = landmarks.merge_workspace_bytes(L_a, L_b)
    assert need == ref.workspace_bytes(L_a, L_b)
    ws = torch.full((max(need, 1),), ws_fill, dtype=torch.uint8, device=dev) if workspace is None else workspace
    p = engine._ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # (the inputs were filled on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = lib.sgpr_landmark_merge(
            *[p(a[k]) if L_a else None for k in ref.RECORD], p(keeps[0]) if L_a else None, L_a,
            *[p(b[k]) if L_b else None for k in ref.RECORD], p(keeps[1]) if L_b else None, L_b,
            None if pose is None else pose.ctypes.data, int(kw.get("session_shift", 0)), int(kw.get("first_base", 0)),
            rad.ctypes.data, rad.size, float(kw.get("tau_z", 0.75)), cap, *[p(out[k]) for k in ref.RECORD], p(out["old_to_new"]),
            p(out["num"]), p(ws), need, engine._stream(dev))
    assert rc == 0, lib.sgpr_last_error()
    return {"out": out, "cap": cap, "T": T, "a": a, "b": b, "keeps": keeps, "case": case, "ws": ws,
            "out_fill": out_fill}


def finish(run):
    """-> the reference's outputs, after the device's were found equal to them to the bit (NaN as NaN: bytes), nothing
    written past the records found or past any output, and the inputs unchanged"""
    torch.cuda.synchronize()
    case, cap, T, out_fill = run["case"], run["cap"], run["T"], run["out_fill"]
    want = ref.run(case, max_out=cap)
    got = {k: v.cpu().numpy() for k, v in run["out"].items()}
    got["sessions"] = got["sessions"].view(np.uint64)
    if T == 0:                                                   # nothing is written
        assert all((v.view(np.uint8) == out_fill).all() for v in got.values())
        return want
    rows = min(int(want["num"][0]), cap)
    for name in ref.RECORD:
        w = 3 if name == "center" else 1
        assert len(want[name]) == rows
        assert got[name][:w * rows].tobytes() == np.ascontiguousarray(want[name], HOST[name]).tobytes(), \
            (name, got[name][:w * rows], want[name].reshape(-1))
        assert (got[name][w * rows:].view(np.uint8) == out_fill).all(), name + ": written past the records"
    for name, n in (("old_to_new", T), ("num", 4)):
        assert got[name][:n].tobytes() == want[name].tobytes(), (name, got[name][:n], want[name].reshape(-1))
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"
    for lm, dev_lm in ((case["a"], run["a"]), (case["b"], run["b"])):
        if lm is not None:
            for k in ref.RECORD:
                assert dev_lm[k].cpu().numpy().tobytes() == np.ascontiguousarray(lm[k], HOST[k]).tobytes(), "input changed: " + k
    for name, mask in zip(("keep_a", "keep_b"), run["keeps"]):
        if mask is not None:
            assert mask.cpu().numpy().tobytes() == np.ascontiguousarray(case["kw"][name], np.uint8).tobytes()
    return want


def check(case, **kw):
    return finish(launch(case, **kw))


def with_kw(case, **over):
    kw = dict(case["kw"])
    kw.update(over)
    return {"a": case["a"], "b": case["b"], "kw": kw}


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 255, 256, 257, 5000])
def test_sizes(T):
    """one record; a wave exact and ragged; a 256-thread block exact and ragged; 5000: twenty blocks for the numbering
    scan and a cell table of 16384 slots"""
    L_a = (T + 1) // 2
    case = ref.random_case(L_a, T - L_a, 100 + T)
    want = check(case)
    if T >= 255:
        assert want["num"][3] >= 3 and want["num"][1] >= 1 and want["num"][2] >= 1 and 0 < want["num"][0] < T
    check(ref.random_case(T, 0, 200 + T, keep=False))            # a compaction
    check(with_kw(case, radius=[0.75, 0.0, 2.0], tau_z=0.3, n_labels=3))


def test_numbering_scan_with_segments_of_two_workgroups():
    """1025 workgroups of 256 records: every thread of the one-workgroup numbering scan owns a SEGMENT of two workgroup
    counts, which no smaller merge reaches.  The expected values are closed forms, not the reference's (its pure-Python
    linking would take minutes here): the input records lie on a lattice of pitch 2 > radius (B's through an integer
    translation), so every kept eligible record is copied - but for three planted pairs 0.5 apart with counts 1 and
    spreads 0: across the workgroups 0 | 1 (255, 256: inside thread 0's segment), across the workgroups 601 | 602
    (154111, 154112: the last of thread 300's segment, the first of thread 301's) and across the maps (199999, 200000).
    263 records are dropped at the indices 100 + 1000 k - by a keep mask and by a count of 0 in turn - so an id is "roots
    before me", never the index."""
    L_a, L_b, ROW, SHIFT, BASE = 200000, 62400, 512, 3, 1 << 20
    T = L_a + L_b
    t = np.arange(T)
    assert T == 1025 * 256
    rec = {"center": np.stack((2.0 * (t % ROW), 2.0 * (t // ROW), 0.125 * (t % 7)), axis=1), "label": (t % 3).astype(np.int32),
           "count": (1 + t % 5).astype(np.int32), "first": ((t * 7) % 100003).astype(np.int32),
           "sessions": (np.uint64(1) << (t % 11).astype(np.uint64)), "spread": 0.25 * (t % 4)}
    pairs = [(255, 256), (602 * 256 - 1, 602 * 256), (L_a - 1, L_a)]
    for a, b in pairs:
        rec["center"][b] = rec["center"][a] + (0.5, 0.0, 0.0)
        rec["label"][b] = rec["label"][a]
        rec["count"][[a, b]] = 1
        rec["spread"][[a, b]] = 0.0
    drop = np.arange(100, T, 1000)
    masked, unfit = drop[0::2], drop[1::2]
    rec["count"][unfit] = 0
    keep = np.ones(T, np.uint8)
    keep[masked] = 0
    assert drop.size == 263 and not set(drop) & {i + d for pr in pairs for i in pr for d in (-1, 0, 1)}
    lm_a = {k: v[:L_a].copy() for k, v in rec.items()}
    lm_b = {k: v[L_a:].copy() for k, v in rec.items()}
    lm_b["center"][:, 0] -= 4096.0                               # B's frame; the pose brings it back, exactly
    case = {"a": lm_a, "b": lm_b, "kw": dict(keep_a=keep[:L_a], keep_b=keep[L_a:], pose=(1.0, 0.0, 4096.0, 0.0),
                                             session_shift=SHIFT, first_base=BASE)}
    run = launch(case)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in run["out"].items()}
    got["sessions"] = got["sessions"].view(np.uint64)

    rec["first"][L_a:] += BASE                                    # the INPUT RECORDS of B
    rec["sessions"][L_a:] <<= np.uint64(SHIFT)
    live = np.ones(T, bool)
    live[drop] = False
    root = live.copy()
    root[[b for _, b in pairs]] = False
    ids = np.cumsum(root) - 1                                     # of a root: the roots before it
    n_roots = int(root.sum())
    assert got["num"][:4].tolist() == [n_roots, masked.size, unfit.size, len(pairs)] and n_roots == T - 263 - 3
    old_to_new = np.where(root, ids, -1).astype(np.int32)
    for a, b in pairs:
        old_to_new[b] = ids[a]
    assert got["old_to_new"][:T].tobytes() == old_to_new.tobytes()
    r = np.flatnonzero(root)
    want = {k: v[r].copy() for k, v in rec.items()}
    for a, b in pairs:
        i = ids[a]
        want["center"][i, 0] += 0.25                              # the mean of x and x + 0.5, weights 1 and 1: exact
        want["count"][i] = 2
        want["first"][i] = min(rec["first"][a], rec["first"][b])
        want["sessions"][i] = rec["sessions"][a] | rec["sessions"][b]
        want["spread"][i] = 0.25                                  # sqrt of the mean of 0^2 + 0.25^2 twice
    for a, b in pairs:                                            # the planted pairs and their neighbours, by name first
        for j in (a - 1, a, b + 1):
            for name in ref.RECORD:
                w = 3 if name == "center" else 1
                assert got[name][w * ids[j]:w * (ids[j] + 1)].tobytes() == want[name][ids[j]].tobytes(), (name, j)
    for name in ref.RECORD:
        w = 3 if name == "center" else 1
        assert got[name][:w * n_roots].tobytes() == np.ascontiguousarray(want[name], HOST[name]).tobytes(), name
        assert (got[name][w * n_roots:].view(np.uint8) == 0xFF).all(), name + ": written past the records"
    for name, n in (("old_to_new", T), ("num", 4)):
        assert (got[name][n:].view(np.uint8) == 0xFF).all(), name + ": written past the output"


def test_hand_made_cases():
    for name, case in ref.hand_cases().items():
        check(case, max_out=case["kw"].get("max_out"))


def test_mutant_cases():
    for name, (case, _) in ref.mutant_cases().items():
        check(case)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("pose", ["null", "identity", "general"])
def test_keep_masks_and_poses(keep, pose):
    case = ref.random_case(300, 260, 7, with_pose=(pose == "general"), keep=keep)
    if pose == "identity":
        case = with_kw(case, pose=(1.0, 0.0, 0.0, 0.0))
        case["b"]["center"][:5, 0] = -0.0                        # the identity pose turns these into +0.0, no pose does not
    want = check(case)
    assert want["num"][3] > 20 and (want["num"][1] > 0) == keep


def test_capacity():
    """max_out 0 - only old_to_new and d_num tell of the landmarks -, one short, exact, ample"""
    case = ref.random_case(400, 300, 5)
    total = int(ref.run(case)["num"][0])
    assert 100 < total < 700
    for cap in (0, total - 1, total, total + 9):
        want = check(case, max_out=cap)
        assert want["num"][0] == total and want["old_to_new"].max() == total - 1 and len(want["label"]) == min(cap, total)


# ------------------------------------------------------------------ structural points of the kernels
def test_1024_records_in_one_component():
    """contention: every record adds to one root's accumulators, the same bits"""
    rng = np.random.default_rng(11)
    c = np.concatenate((rng.normal(0.0, 0.15, size=(1024, 2)), rng.uniform(-0.3, 0.3, size=(1024, 1))), axis=1)
    lm = ref.lm_of(c, [2] * 1024, count=rng.integers(1, 50, 1024), first=rng.integers(0, 1 << 20, 1024),
                   sessions=rng.integers(1, 1 << 40, 1024), spread=rng.uniform(0.0, 0.3, 1024))
    a = {k: v[:600] for k, v in lm.items()}
    b = {k: v[600:] for k, v in lm.items()}
    want = check({"a": a, "b": b, "kw": dict(session_shift=5, first_base=77)})
    assert want["num"].tolist() == [1, 0, 0, 1] and want["count"].tolist() == [int(lm["count"].sum())]


def test_a_chain_of_300_records():
    """union-find depth: each record links its two neighbours only, the last joins the first through all of them"""
    order = np.random.default_rng(3).permutation(300)
    lm = ref.lm_of([(0.7 * int(i), 0.0, 0.0) for i in order], [0] * 300, count=[1 + int(i) % 5 for i in order])
    want = check({"a": lm, "b": None, "kw": {}})
    assert want["num"].tolist() == [1, 0, 0, 1] and want["links"] == 299
    straight = ref.lm_of([(0.7 * i, 0.0, 0.0) for i in range(300)], [0] * 300)
    check({"a": {k: v[:150] for k, v in straight.items()}, "b": {k: v[150:] for k, v in straight.items()}, "kw": {}})


def test_4000_singletons():
    """the numbering scan across its block boundaries: every record keeps its id and its bits"""
    rng = np.random.default_rng(8)
    g = np.stack(np.meshgrid(np.arange(80), np.arange(50)), axis=-1).reshape(-1, 2) * 3.0
    lm = ref.lm_of(np.concatenate((g, rng.uniform(-1, 1, (4000, 1))), axis=1), rng.integers(0, 12, 4000), count=rng.integers(1, 9, 4000),
                   first=rng.integers(0, 1 << 30, 4000), sessions=rng.integers(1, 1 << 62, 4000), spread=rng.uniform(0, 1, 4000))
    keep = (rng.random(4000) >= 0.25).astype(np.uint8)
    want = check({"a": lm, "b": None, "kw": {}})
    assert want["num"].tolist() == [4000, 0, 0, 0] and want["old_to_new"].tolist() == list(range(4000))
    assert all(want[k].tobytes() == lm[k].tobytes() for k in ref.RECORD)
    want = check({"a": lm, "b": None, "kw": dict(keep_a=keep)})
    ids = np.flatnonzero(keep)
    assert want["num"][0] == ids.size and all(want[k].tobytes() == lm[k][ids].tobytes() for k in ref.RECORD)


def test_cells_that_share_a_key_share_a_list_and_change_nothing():
    """landmark_merge_ref.COLLIDING_CELLS: three cells of label 0 with one key, two of label 1 with another.  Records that
    fuse and records that do not lie in every one of them and in the cells beside them, so a shared list is walked from
    inside and is met among the nine neighbours of the records beside it.  The keys the kernels left in the cell table
    are read back from the workspace: they are the reference's keys, fewer than the cells that hold a record."""
    case = ref.collision_case()
    run = launch(case)
    want = finish(run)
    n_cells = sum(len(cells) for _, cells in ref.COLLIDING_CELLS)
    assert want["num"].tolist() == [4 * n_cells, 0, 0, 2 * n_cells] and run["T"] == 6 * n_cells
    rec, _ = ref.input_records(case["a"], case["b"])
    w = ref.cell_width(0.75)
    cells = {(int(l), ref.cell_coord(c[0], w), ref.cell_coord(c[1], w)) for c, l in zip(rec["center"], rec["label"])}
    keys = {ref.cell_key(*cell) for cell in cells}
    T = run["T"]
    al = lambda v: (v + 255) & ~255                              # noqa: E731  (the table follows the per-record arrays)
    start = 3 * al(24 * T) + 3 * al(8 * T) + 6 * al(4 * T)
    table = run["ws"][start:start + 8 * 1024].cpu().numpy().view(np.uint64)
    on_device = set(table[table != np.uint64(0xffffffffffffffff)].tolist())
    assert on_device == keys and len(cells) == 3 * n_cells and len(keys) == len(cells) - (n_cells - len(ref.COLLIDING_CELLS))
    # with the maps exchanged (other indices, other list orders), and with every second record of A masked out
    check({"a": case["b"], "b": case["a"], "kw": case["kw"]})
    check(with_kw(case, keep_a=(np.arange(len(case["a"]["label"])) % 2).astype(np.uint8)))


def test_every_record_in_a_cell_of_its_own_fills_the_table_to_its_limit():
    """512 records, 512 distinct cell keys in the 1024 slots the table has at the least: the fullest table the sizing
    rule allows, with the longest probe runs; and 513, where the table doubles."""
    for n in (512, 513):
        g = np.stack(np.meshgrid(np.arange(32), np.arange(17)), axis=-1).reshape(-1, 2)[:n] * 0.76
        lm = ref.lm_of(np.concatenate((g, np.zeros((n, 1))), axis=1), [0] * n)
        want = check({"a": lm, "b": None, "kw": {}})
        assert want["num"][0] == n
        pairs = ref.lm_of(np.concatenate((g + 0.01, np.zeros((n, 1))), axis=1), [0] * n)
        want = check({"a": lm, "b": pairs, "kw": dict(session_shift=1)})
        assert want["num"].tolist() == [n, 0, 0, n]


def test_all_records_dropped():
    case = ref.random_case(200, 100, 9)
    want = check(with_kw(case, keep_a=np.zeros(200, np.uint8), keep_b=np.zeros(100, np.uint8)))
    assert want["num"].tolist() == [0, 300, 0, 0] and (want["old_to_new"] == -1).all()
    bad = ref.random_case(200, 100, 9, keep=False)
    bad["a"]["count"][:] = 0
    bad["b"]["spread"][:] = np.nan
    want = check(bad)
    assert want["num"].tolist() == [0, 0, 300, 0]
    check({"a": ref.lm_of(np.zeros((0, 3)), []), "b": None, "kw": {}})             # no record at all: nothing is written


# ------------------------------------------------------------------ streams and workspaces
def test_two_streams_with_different_inputs_at_once():
    x, y = ref.random_case(2500, 2500, 21), ref.random_case(1800, 2200, 22, with_pose=False)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    r1 = launch(x, stream=s1)
    r2 = launch(y, stream=s2)
    finish(r1)
    finish(r2)


def test_a_workspace_used_twice():
    case, other = ref.random_case(700, 400, 6), ref.random_case(600, 500, 7)
    ws = torch.full((ref.workspace_bytes(700, 400),), 0xFF, dtype=torch.uint8, device="cuda")
    check(case, workspace=ws)
    check(case, workspace=ws)                                    # dirty with the first call's state
    check(other, workspace=ws)


# ------------------------------------------------------------------ the Python layer
def test_python_layer():
    from sg_pr_amd import landmarks
    case = ref.random_case(500, 400, 4)
    kw = {k: v for k, v in case["kw"].items() if k != "n_labels"}
    want = ref.run(case)
    dev = torch.device("cuda", 0)
    a, b = to_device(case["a"], dev), to_device(case["b"], dev)
    a["center"], b["center"] = a["center"].reshape(-1, 3), b["center"].reshape(-1, 3)
    got = landmarks.merge(a, b, **kw)
    for k in ref.RECORD + ("old_to_new",):
        assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert [got["num_landmarks"], *got["dropped"], got["fused"]] == want["num"].tolist()
    assert a["count"].cpu().numpy().tobytes() == case["a"]["count"].tobytes()      # the input maps are left as they are
    # a capacity that is too small is repaired by a second call; host arrays are taken too
    got = landmarks.merge(case["a"], case["b"], max_landmarks=10, **kw)
    assert got["num_landmarks"] == want["num"][0] and got["spread"].cpu().numpy().tobytes() == want["spread"].tobytes()
    raw = landmarks.merge_async(a, b, max_landmarks=10, **kw)
    assert raw["num"].tolist() == want["num"].tolist() and raw["label"].shape[0] == 10
    short = torch.empty(landmarks.merge_workspace_bytes(500, 400) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception, match="workspace"):
        landmarks.merge_async(a, b, workspace=short, **kw)
    # a session bit shifted out: merge raises, merge_async does not
    lost = dict(b, sessions=b["sessions"] | (1 << 62))
    with pytest.raises(ValueError, match="session"):
        landmarks.merge(a, lost, **kw)
    assert landmarks.merge_async(a, lost, **kw)["num"].tolist() == want["num"].tolist()
    # compact = merge with no b; an empty map
    only = landmarks.compact(a, keep=case["kw"]["keep_a"], radius=0.75)
    want_a = ref.merge(case["a"], None, keep_a=case["kw"]["keep_a"])
    assert all(only[k].cpu().numpy().tobytes() == want_a[k].tobytes() for k in ref.RECORD + ("old_to_new",))
    none = landmarks.merge({k: v[:0] for k, v in a.items()})
    assert none["num_landmarks"] == 0 and none["old_to_new"].numel() == 0 and none["center"].shape == (0, 3)
    node = torch.as_tensor(np.array([[0, 5, -1, -2, 499]], np.int32)).cuda()
    assert landmarks.remap(node, only["old_to_new"]).cpu().numpy().tolist() == ref.remap(node.cpu().numpy(), want_a["old_to_new"]).tolist()


def test_a_merged_map_feeds_select_align_update_persist_and_virtual_scans():
    from sg_pr_amd import landmarks
    c, l, p, _, lm = uref.make_case(5, 130, 300, 4)
    half = {k: v[:150] for k, v in lm.items()}, {k: v[150:] for k, v in lm.items()}
    want = ref.merge(*half, session_shift=2, first_base=5000)
    got = landmarks.merge(*half, session_shift=2, first_base=5000)
    keep = landmarks.select(got, min_count=3)
    assert keep.shape[0] == got["num_landmarks"] == want["num"][0] and 0 < int(keep.sum()) < keep.shape[0]
    X, info = landmarks.align(c, l, p, got, use=keep, iters=2)
    host = aref.align(c, l, p, want["center"], want["label"], lm_use=keep.cpu().numpy().astype(np.uint8), iters=2)
    assert X.cpu().numpy().tobytes() == host["poses"].tobytes() and info["node_landmark"].tobytes() == host["node_landmark"].tobytes()
    assoc = landmarks.align_async(c, l, p, got, iters=0)["node_landmark"]
    up = landmarks.update(c, l, p, assoc, got, session_base=4, node_base=9000)
    want_up = uref.update(c, l, p, assoc.cpu().numpy(), want, session_base=4, node_base=9000)
    assert all(up[k].cpu().numpy().tobytes() == want_up[k].tobytes() for k in ref.RECORD) and up["observed"] > 300
    tally = landmarks.persist(c, l, p, up["node_landmark"], up, max_range=14.0, margin=1.0, min_expected=3)
    want_t = pref.persist(c, l, p, want_up["node_landmark"], want_up, max_range=14.0, margin=1.0, min_expected=3)
    assert tally["keep"].cpu().numpy().astype(np.uint8).tolist() == want_t["keep"].tolist()
    again = landmarks.compact(up, keep=tally["keep"])
    want_c = ref.merge(want_up, None, keep_a=want_t["keep"])
    assert all(again[k].cpu().numpy().tobytes() == want_c[k].tobytes() for k in ref.RECORD + ("old_to_new",))
    vc, vl = landmarks.virtual_scans(got, p[:2], keep=keep)
    hc, hl = lref.virtual_scans(want["center"], want["label"], p[:2], keep=keep.cpu().numpy())
    assert vl.cpu().numpy().tolist() == hl.tolist() and np.allclose(vc.cpu().numpy(), hc, atol=1e-5) and (hl >= 0).any()


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


def test_register_maps_and_merge_maps(model):
    """the planted world cut to 70 scans a drive: drive 1's map, built in a frame of its own, is registered in drive 0's
    from the landmarks alone and merged; both equal the reference composition to the bit"""
    from sg_pr_amd import synth
    w = synth.landmark_world(0, scans=70)
    N = w["labels"].shape[1]
    yaw, X, Y = 0.9, 300.0, -120.0
    frame = np.array([np.cos(yaw), np.sin(yaw), X, Y])
    inv = np.array([frame[0], -frame[1], -(frame[0] * X + frame[1] * Y), frame[1] * X - frame[0] * Y])
    own = np.stack([ref.compose(inv, q) for q in w["truth"][70:140]])
    A = model.landmark_map(w["centers"][:70], w["labels"][:70], w["truth"][:70])
    B = model.landmark_map(w["centers"][70:140], w["labels"][70:140], own)
    hA = lref.landmark_map(w["centers"][:70], w["labels"][:70], w["truth"][:70])
    hB = lref.landmark_map(w["centers"][70:140], w["labels"][70:140], own)
    want_pose, want_info = ref.register(hA, hB)
    pose, info = model.register_maps(A, B)
    assert want_pose is not None and pose is not None and info["found"] and not info["ambiguous"]
    assert {k: info[k] for k in want_info} == want_info and pose.tobytes() == want_pose.tobytes()
    assert np.hypot(pose[2] - X, pose[3] - Y) < 0.1 and np.abs(pose[:2] - frame[:2]).max() < 1e-3
    got = model.merge_maps(A, B, pose="register")
    want = ref.merge(hA, hB, pose=want_pose, session_shift=1, first_base=int(hA["first"].max()) + 1)
    for k in ref.RECORD + ("old_to_new",):
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert [got["num_landmarks"], *got["dropped"], got["fused"]] == want["num"].tolist() and got["pose"].tobytes() == pose.tobytes()
    assert want["num"][3] > 30 and want["num"][0] < hA["count"].size + hB["count"].size
    assert set(got["sessions"].cpu().numpy().tolist()) == {1, 2, 3}
    # a pose given, one frame, a compaction; a B that cannot be found
    same = model.merge_maps(A, model.landmark_map(w["centers"][70:140], w["labels"][70:140], w["truth"][70:140]))
    assert same["pose"] is None and same["fused"] > 30
    small = model.compact_map(got, keep=got["count"] >= 3)
    assert small["dropped"] == (int((got["count"] < 3).sum()), 0) and small["dropped"][0] > 0
    assert 0 < small["num_landmarks"] <= int((got["count"] >= 3).sum()) and int(small["count"].min()) >= 3
    none, info = model.register_maps(A, B, min_inliers=10 ** 6)
    assert none is None and not info["found"]
    with pytest.raises(RuntimeError, match="registered"):
        model.merge_maps(A, B, pose="register", min_inliers=10 ** 6)


def _config(tmp_path, ckpt_path):
    from sg_pr_amd import graph_store, synth
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
    return cfg, centers, labels, poses


def test_place_db_compact_cli(model, tmp_path, ckpt_path, capsys):
    """--update --retire --compact: the file holds the reference's compaction of the updated map under the retire mask"""
    from sg_pr_amd import place_db
    cfg, centers, labels, poses = _config(tmp_path, ckpt_path)
    place_db.main([str(cfg), "--k", "3", "--window", "14", "--landmarks", "--sessions", "3", "--update", "--retire", "--compact",
                   "--align-radii", "1.5,0.75", "--align-iters", "4", "--view-range", "30", "--min-expected", "3"])
    lines = capsys.readouterr().out.splitlines()
    u, pz, z = (np.load(tmp_path / "eva" / ("07_%s.npz" % n)) for n in ("update", "persist", "compact"))
    up = {k: u[k] for k in ref.RECORD}
    up["sessions"] = up["sessions"].view(np.uint64)
    want = ref.merge(up, None, keep_a=pz["keep"])
    for k in ref.RECORD + ("old_to_new",):
        assert z[k].view(want[k].dtype).tobytes() == want[k].tobytes(), k
    assert z["num"].tolist() == want["num"].tolist() and int(z["landmarks_before"]) == len(u["count"])
    assert z["node_landmark"].tolist() == ref.remap(u["node_landmark"], want["old_to_new"]).tolist()
    assert z["num"][1] == (~pz["keep"]).sum() and z["num"][0] == len(z["count"]) <= len(u["count"]) - z["num"][1]
    line = next(t for t in lines if "compacted on its records" in t)
    assert "landmarks %d -> %d, dropped %d, fused %d" % (len(u["count"]), z["num"][0], z["num"][1] + z["num"][2], z["num"][3]) in line
    assert "under the retire mask" in line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--landmarks", "--sessions", "3", "--compact"])


def test_place_db_merge_maps_cli(model, tmp_path, ckpt_path, capsys):
    """--landmarks --sessions 3 --merge-maps: one map per session on the sequence's own poses, merged left to right"""
    from sg_pr_amd import metrics, place_db
    cfg, centers, labels, poses = _config(tmp_path, ckpt_path)
    place_db.main([str(cfg), "--k", "3", "--window", "14", "--landmarks", "--sessions", "3", "--merge-maps"])
    lines = capsys.readouterr().out.splitlines()
    own = metrics.planar_odometry(poses)
    maps = [lref.landmark_map(centers[lo:lo + 30], labels[lo:lo + 30], own[lo:lo + 30]) for lo in (0, 30, 60)]
    want = maps[0]
    for j in (1, 2):
        want = ref.merge(want, maps[j], session_shift=j, first_base=30 * j * 100)
    z = np.load(tmp_path / "eva" / "07_merge.npz")
    for k in ref.RECORD:
        assert z[k].view(want[k].dtype).tobytes() == want[k].tobytes(), k
    batch = lref.landmark_map(centers, labels, own, starts=[0, 30, 60])
    same = batch["count"][batch["node_landmark"].reshape(-1)[want["first"]]] == want["count"]
    assert z["num"].tolist() == want["num"].tolist() and z["landmarks_per_session"].tolist() == [len(m["count"]) for m in maps]
    assert int(z["batch_landmarks"]) == batch["num"][0] and abs(float(z["same_count"]) - same.mean()) < 1e-12
    assert z["count"].sum() == batch["num"][1]
    line = next(t for t in lines if "merged on their records" in t)
    assert "-> %d, fused" % want["num"][0] in line and "has %d landmarks" % batch["num"][0] in line
    with pytest.raises(SystemExit):
        place_db.main([str(cfg), "--merge-maps"])
