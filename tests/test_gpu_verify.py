"""sgpr_verify_pairs on the MI355X: every record against tests/geo_ref.py BIT FOR BIT, field by field (NaN payloads
compare as NaN) - world pairs, edge graphs, the cap, bad indices, statelessness - and the Python surface on top of it
(SG.verify_closures, metrics.closure_pose_errors, the place_db --verify CLI, tools/verify_bench.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_ref  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_records(ca, la, cb, lb, ia, ib, **tol):
    from sg_pr_amd import engine
    if "tau_in" in tol:
        tol["tau_inlier"] = tol.pop("tau_in")
    out = engine.verify_pairs(np.asarray(ca, np.float32), np.asarray(la, np.int32), np.asarray(cb, np.float32),
                              np.asarray(lb, np.int32), np.asarray(ia, np.int32), np.asarray(ib, np.int32), **tol)
    torch.cuda.synchronize()
    return out["record"].cpu().numpy().view(engine.VERIFY_RESULT).reshape(-1), out


def check(ca, la, cb, lb, ia, ib, **tol):
    got, fields = gpu_records(ca, la, cb, lb, ia, ib, **tol)
    want = geo_ref.verify_pairs(ca, la, cb, lb, ia, ib, **tol)
    bad = geo_ref.equal_records(got, want)
    if bad:
        n = next(i for i in range(len(got)) if geo_ref.equal_records(got[i:i + 1], want[i:i + 1]))
        raise AssertionError("fields %s differ; first at pair %d (%d, %d):\n gpu %s\n ref %s" % (bad, n, ia[n], ib[n], got[n], want[n]))
    # the dict of fields is the record, field by field
    for name in geo_ref.RESULT.names:
        assert np.array_equal(fields[name].cpu().numpy().astype(got[name].dtype), got[name], equal_nan=True), name
    assert np.allclose(fields["yaw"].cpu().numpy(), np.arctan2(got["refined"][:, 1], got["refined"][:, 0]), rtol=0, atol=1e-12,
                       equal_nan=True)
    return got


# ------------------------------------------------------------------ 1. world pairs
def _world_pairs():
    t = np.arange(60, 90)
    ia = np.concatenate([t, np.arange(30), [0, 29, 45, 89]])           # 30 revisits, 30 non-revisits, 4 identity pairs
    ib = np.concatenate([t - 60, (np.arange(30) + 37) % 60, [0, 29, 45, 89]])
    return ia, ib


def test_world_pairs_n100():
    from sg_pr_amd import synth
    centers, labels, n_real, _ = synth.world_sequence(90, 100, seed=3)
    ia, ib = _world_pairs()
    got = check(centers, labels, centers, labels, ia, ib)
    assert (got["flags"] == 0).all()
    assert (got["inliers"][:30] >= 0.7 * np.minimum(n_real[ia[:30]], n_real[ib[:30]])).all()    # revisits are found
    assert (got["inliers"][60:] == n_real[ia[60:]]).all()                                      # a scan against itself


def test_world_pairs_n64_with_full_graphs():
    from sg_pr_amd import synth
    centers, labels, n_real, _ = synth.world_sequence(90, 104, seed=3, sensor_range=60.0)
    assert (n_real == 64).any()                        # node_num - 40 = 64 real nodes: no padding slot at N = 64
    centers, labels = np.ascontiguousarray(centers[:, :64]), np.ascontiguousarray(labels[:, :64])
    assert (labels >= 0).all(axis=1).any()
    ia, ib = _world_pairs()
    got = check(centers, labels, centers, labels, ia, ib)
    assert (got["flags"] == 0).all() and (got["inliers"][60:] == n_real[ia[60:]]).all()


# ------------------------------------------------------------------ 2. edge graphs
def _graph(n_slots, nodes):
    """nodes: list of (slot, x, y, z, label)"""
    c = np.zeros((n_slots, 3), np.float32)
    lab = -np.ones(n_slots, np.int32)
    for slot, x, y, z, l in nodes:
        c[slot] = (x, y, z)
        lab[slot] = l
    return c, lab


def _random_graph(rng, n_slots, n, labels, box=40.0, shuffle_slots=True):
    slots = rng.permutation(n_slots)[:n] if shuffle_slots else np.arange(n)
    xy = rng.uniform(-box, box, (n, 2))
    z = rng.uniform(-2, 1, n)
    lab = rng.choice(np.asarray(labels), n)
    return _graph(n_slots, [(s, x, y, zz, l) for s, (x, y), zz, l in zip(slots, xy, z, lab)])


def _moved(rng, c, lab, yaw, t, noise=0.05):
    """The graph rotated, translated and jittered, its nodes in permuted slots."""
    n_slots = len(lab)
    real = np.flatnonzero(lab >= 0)
    slots = rng.permutation(n_slots)[:real.size]
    out_c, out_l = np.zeros_like(c), -np.ones_like(lab)
    cs, sn = np.cos(yaw), np.sin(yaw)
    x, y = c[real, 0].astype(np.float64), c[real, 1].astype(np.float64)
    out_c[slots, 0] = cs * x - sn * y + t[0] + rng.normal(0, noise, real.size)
    out_c[slots, 1] = sn * x + cs * y + t[1] + rng.normal(0, noise, real.size)
    out_c[slots, 2] = c[real, 2]
    out_l[slots] = lab[real]
    return out_c, out_l


def test_edge_graphs_in_one_call():
    rng = np.random.default_rng(11)
    N = 100
    g = []
    g.append(_graph(N, []))                                                          # 0 all padding
    g.append(_graph(N, [(17, 1.0, 2.0, 0.5, 3)]))                                   # 1 one real node
    g.append(_graph(N, [(2, 0.0, 0.0, 0.0, 1), (9, 3.0, 0.0, 0.0, 1)]))            # 2 two nodes closer than min_base
    dup = [(s, 10.0, -4.0, 0.25, 2) for s in (0, 5, 6)] + [(s, -8.0, 6.0, 0.0, 2) for s in (20, 21)] + \
          [(40, 12.0, 12.0, 0.0, 4), (41, 12.0, 12.0, 0.0, 4), (60, -15.0, 2.0, -1.0, 4)]
    g.append(_graph(N, dup))                                                         # 3 duplicated nodes (lv == 0)
    base = _random_graph(rng, N, 30, [0, 1, 2, 3, 4])
    nan_c = base[0].copy()
    nan_c[np.flatnonzero(base[1] >= 0)[4], 2] = np.nan
    inf_c = base[0].copy()
    inf_c[np.flatnonzero(base[1] >= 0)[7], 0] = -np.inf
    g.append((nan_c, base[1]))                                                       # 4 a NaN centre
    g.append((inf_c, base[1]))                                                       # 5 an inf centre
    g.append(_graph(N, [(3, 0, 0, 0, 5), (30, 10, 0, 0, 5), (31, 10, 10, 0, 5), (77, 0, 10, 0, 5)]))   # 6 square: ties
    g.append(_random_graph(rng, N, 45, [1000, 7, 0, 2 ** 31 - 1, 12, 3]))            # 7 labels in no order, large values
    g.append(base)                                                                   # 8 an ordinary graph
    g.append(_moved(rng, *base, yaw=2.5, t=(-7.0, 11.0)))                            # 9 ... seen from elsewhere
    g.append(_moved(rng, *g[7], yaw=-1.1, t=(4.0, 0.5)))                             # 10 graph 7 seen from elsewhere
    pad_junk = (base[0].copy(), base[1])
    pad_junk[0][base[1] < 0] = np.nan                                                # 11 padding slots hold NaN: ignored
    g.append(pad_junk)
    centers = np.stack([c for c, _ in g])
    labels = np.stack([l for _, l in g])
    pairs = [(0, 0), (0, 8), (8, 0), (1, 1), (1, 8), (8, 1), (2, 2), (3, 3), (3, 8), (4, 8), (8, 5), (4, 4), (5, 0), (0, 4),
             (6, 6), (7, 7), (7, 10), (10, 7), (8, 9), (9, 8), (8, 8), (11, 9), (9, 11), (7, 8)]
    ia, ib = np.array(pairs).T
    got = check(centers, labels, centers, labels, ia, ib)
    f = dict(zip(pairs, got))
    NOH, NONF = geo_ref.NO_HYPOTHESIS, geo_ref.NONFINITE
    assert [f[p]["flags"] for p in ((0, 0), (0, 8), (8, 0), (1, 1), (1, 8), (2, 2))] == [NOH] * 6
    assert [f[p]["flags"] for p in ((4, 8), (8, 5), (4, 4), (5, 0), (0, 4))] == [NONF] * 5
    assert f[(3, 3)]["flags"] == 0 and f[(3, 3)]["inliers"] == 8
    # the square against itself: four rotations reach 4 inliers; the lowest (i, i', j, j') is the identity on (3, 30)
    assert f[(6, 6)]["inliers"] == 4 and f[(6, 6)]["base"].tolist() == [3, 30, 3, 30]
    assert f[(7, 10)]["inliers"] >= 40 and f[(8, 9)]["inliers"] >= 27
    assert geo_ref.equal_records(got[[18]], got[[21]]) == [] and f[(11, 9)]["flags"] == 0    # (8, 9) and (11, 9)
    # a finer world: other tolerances, same bits as the reference
    check(centers, labels, centers, labels, ia, ib, tau_edge=0.25, tau_in=0.3, tau_z=0.5, min_base=0.0, max_hyp=300)


def test_n1_and_n256():
    c1 = np.array([[[1, 2, 3]], [[0, 0, 0]]], np.float32)
    l1 = np.array([[4], [-1]], np.int32)
    got = check(c1, l1, c1, l1, [0, 0, 1, 1], [0, 1, 0, 1])
    assert (got["flags"] == geo_ref.NO_HYPOTHESIS).all()
    rng = np.random.default_rng(5)
    a = _random_graph(rng, 256, 256, np.arange(40), box=80.0)
    b = _moved(rng, *a, yaw=0.4, t=(2.0, -3.0))
    centers, labels = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
    got = check(centers, labels, centers, labels, [0, 1, 0], [1, 0, 0], max_hyp=2000)
    assert (got["flags"] == geo_ref.TRUNCATED).all() and (got["hypotheses"] >= 2000).all()
    assert got["inliers"][2] == 256 and got["inliers"][0] >= 200


# ------------------------------------------------------------------ 3. the cap
@pytest.mark.parametrize("max_hyp", [1, 500, 1 << 20])
def test_cap_single_label_48_nodes(max_hyp):
    rng = np.random.default_rng(48)
    a = _random_graph(rng, 64, 48, [2], box=150.0)
    b = _moved(rng, *a, yaw=1.0, t=(5.0, 5.0), noise=0.1)
    centers, labels = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
    got = check(centers, labels, centers, labels, [0, 1], [1, 0], max_hyp=max_hyp)
    if max_hyp <= 500:
        assert (got["flags"] == geo_ref.TRUNCATED).all() and (got["hypotheses"] >= max_hyp).all()
        assert (got["hypotheses"] < max_hyp + 48 * 47).all()       # one base pair adds at most nB^2 past the cap
    else:
        assert (got["flags"] == 0).all() and (got["hypotheses"] > 500).all()


def test_cap_256_slots_12_labels():
    rng = np.random.default_rng(256)
    a = _random_graph(rng, 256, 256, np.arange(12), box=60.0)
    b = _random_graph(rng, 256, 250, np.arange(12), box=60.0)
    centers, labels = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
    got = check(centers, labels, centers, labels, [0, 1, 1], [1, 0, 1], max_hyp=3000)
    assert (got["flags"] == geo_ref.TRUNCATED).all() and (got["hypotheses"] >= 3000).all()


# ------------------------------------------------------------------ 4. indices
def test_bad_indices_are_flagged_and_touch_nothing_else():
    from sg_pr_amd import engine, synth
    ca, la, _, _ = synth.world_sequence(12, 100, seed=9)
    cb, lb = ca[:7], la[:7]                                           # GA = 12, GB = 7
    good = [(3, 2), (11, 6), (0, 0), (5, 5)]
    mixed = [(3, 2), (-1, 2), (11, 6), (12, 0), (0, 0), (0, 7), (0, -1), (5, 5), (2 ** 31 - 1, 0), (-2 ** 31, -2 ** 31)]
    g0, _ = gpu_records(ca, la, cb, lb, *np.array(good).T)
    g1, _ = gpu_records(ca, la, cb, lb, *np.array(mixed).T)
    keep = [0, 2, 4, 7]
    assert g1[keep].tobytes() == g0.tobytes()
    flagged = np.delete(g1, keep)
    want = np.zeros(len(flagged), dtype=engine.VERIFY_RESULT)
    want["flags"] = engine.VERIFY_INVALID_INDEX
    assert flagged.tobytes() == want.tobytes()
    assert geo_ref.equal_records(g1, geo_ref.verify_pairs(ca, la, cb, lb, *np.array(mixed).T)) == []
    # P = 0
    out = engine.verify_pairs(ca, la, cb, lb, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert out["record"].shape == (0, 88) and out["inliers"].numel() == 0 and out["yaw"].numel() == 0


# ------------------------------------------------------------------ 5. statelessness
def test_two_streams_prefilled_output_equal_bytes():
    from sg_pr_amd import engine, synth
    lib = engine.load_library()
    ca, la, _, _ = synth.world_sequence(9, 100, seed=21)
    GA, GB = 5, 9                                                     # row and column graph sets differ in G
    dca, dla = torch.from_numpy(ca[:GA]).cuda(), torch.from_numpy(la[:GA]).cuda()
    dcb, dlb = torch.from_numpy(ca).cuda(), torch.from_numpy(la).cuda()
    ia = np.array([0, 4, 2, 4, 5, 1, 3], np.int32)                    # (5 is outside the row set, 8 inside the column set)
    ib = np.array([8, 4, 7, 0, 0, 6, 9], np.int32)
    dia, dib = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    outs = []
    torch.cuda.synchronize()
    for fill in (0xFF, 0x00):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out = torch.full((len(ia), 88), fill, dtype=torch.uint8, device="cuda")
            rc = lib.sgpr_verify_pairs(dca.data_ptr(), dla.data_ptr(), GA, dcb.data_ptr(), dlb.data_ptr(), GB, 100,
                                       dia.data_ptr(), dib.data_ptr(), len(ia), 0.5, 0.6, 1.0, 5.0, 65536,
                                       out.data_ptr(), ctypes.c_void_p(s.cuda_stream))
            assert rc == 0, lib.sgpr_last_error()
        outs.append((s, out))
    for s, _ in outs:
        s.synchronize()
    b0, b1 = (o.cpu().numpy().tobytes() for _, o in outs)
    assert b0 == b1
    got = np.frombuffer(b0, dtype=engine.VERIFY_RESULT)
    assert geo_ref.equal_records(got, geo_ref.verify_pairs(ca[:GA], la[:GA], ca, la, ia, ib)) == []
    assert got["flags"].tolist()[4] == 1 and got["flags"].tolist()[6] == 1


# ------------------------------------------------------------------ 6. the Python surface
@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


@pytest.fixture(scope="module")
def small_world():
    from sg_pr_amd import synth
    return synth.world_sequence(90, 100, seed=3)


def test_verify_closures_reranks_and_accepts(model, small_world):
    centers, labels, _, _ = small_world
    pooled = model.embed(centers, labels)[0]
    model.engine().check_status()
    vals, idx = model.loop_closures(pooled, pooled, k=4, window=43)   # 90 frames, window 43: rows 44 and 45 have 3 eligible columns
    assert (idx < 0).any() and (idx >= 0).any()
    out = model.verify_closures(centers, labels, idx, values=vals, min_inliers=12)
    torch.cuda.synchronize()
    idx_h, val_h = idx.cpu().numpy(), vals.cpu().numpy()
    inl = out["inliers_refined"].cpu().numpy()
    assert inl.shape == idx_h.shape and out["refined"].shape == idx_h.shape + (4,)
    flags = out["flags"].cpu().numpy()
    assert ((flags == 1) == (idx_h < 0)).all() and (inl[idx_h < 0] == 0).all()
    # the slots are the records of the flat pair list
    r, k = idx_h.shape
    want = geo_ref.verify_pairs(centers, labels, centers, labels, np.repeat(np.arange(r), k)[:40], idx_h.reshape(-1)[:40])
    got = out["record"].cpu().numpy().reshape(-1, 88)[:40].copy().view(geo_ref.RESULT).reshape(-1)
    assert geo_ref.equal_records(got, want) == []
    # the order is a NumPy sort of the returned fields: refined inliers descending, score descending, column ascending
    order = out["order"].cpu().numpy()
    for row in range(r):
        valid = idx_h[row] >= 0
        keys = (np.arange(k), np.where(valid, idx_h[row], 2 ** 31 - 1), -val_h[row].astype(np.float64),
                -np.where(valid, inl[row], -1))
        assert order[row].tolist() == np.lexsort(keys).tolist(), row
    assert np.array_equal(out["indices_ranked"].cpu().numpy(), np.take_along_axis(idx_h, order, 1))
    assert np.array_equal(out["accept"].cpu().numpy(), inl >= 12)
    # other column graphs: the first 50 frames as the map
    out2 = model.verify_closures(centers[60:], labels[60:], np.arange(30, dtype=np.int32)[:, None], col_centers=centers[:50],
                                 col_labels=labels[:50])
    assert (out2["inliers"].cpu().numpy()[:, 0] >= 27).all() and out2["order"].shape == (30, 1) and "accept" not in out2


def test_closure_pose_errors_on_revisits(small_world):
    """The host test's bounds (tests/test_verify_host.py): refined yaw error <= 0.5 deg, translation error <= 0.2 m."""
    from sg_pr_amd import engine, metrics
    centers, labels, n_real, poses = small_world
    rows, cols = np.arange(60, 90), np.arange(0, 30)
    res = engine.verify_pairs(centers, labels, centers, labels, rows, cols)
    e = metrics.closure_pose_errors(res, rows, cols, poses)
    print("yaw <= %.3f deg, translation <= %.3f m, medians %.3f deg %.3f m" % (
        e["yaw_deg"].max(), e["trans_m"].max(), e["median_yaw_deg"], e["median_trans_m"]))
    assert e["yaw_deg"].shape == (30,) and e["yaw_deg"].max() <= 0.5 and e["trans_m"].max() <= 0.2
    assert e["median_yaw_deg"] <= e["yaw_deg"].max() and e["median_trans_m"] <= e["trans_m"].max()
    assert (res["inliers"].cpu().numpy() >= 0.7 * np.minimum(n_real[rows], n_real[cols])).all()
    # a pair without a transform has no error
    bad = metrics.closure_pose_errors(engine.verify_pairs(centers, labels, centers, labels, [3, 4], [-1, 5]), [3, 4], [-1, 5], poses)
    assert np.isnan(bad["yaw_deg"][0]) and np.isfinite(bad["yaw_deg"][1]) and np.isfinite(bad["median_trans_m"])


def _numbers(text):
    import re
    return [float(x) for x in re.findall(r"(?<![\w.])-?\d+\.\d+(?![\w.])", text)]


def test_place_db_verify_cli(model, tmp_path, ckpt_path, capsys):
    from sg_pr_amd import graph_store, place_db, synth
    centers, labels, _, poses = synth.world_sequence(150, 100, seed=4)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(150)])
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
    place_db.main([str(cfg), "--k", "4", "--window", "30", "--verify", "--min-inliers", "15"])
    text = capsys.readouterr().out
    line = next(l for l in text.splitlines() if "verified" in l)
    nums = _numbers(line)
    assert len(nums) >= 5 and np.isfinite(nums).all(), line
    z = np.load(tmp_path / "eva" / "07_verify.npz")
    top = np.load(tmp_path / "eva" / "07_topk.npz")
    assert z["inliers_refined"].shape == (150, 4) and z["refined"].shape == (150, 4, 4)
    assert np.array_equal(z["accept"], (z["inliers_refined"] >= 15) & (top["indices"] >= 0))
    assert np.array_equal(np.sort(z["indices_ranked"], 1), np.sort(top["indices"], 1))
    # scans tens of metres apart still overlap and may verify as well: precision is reported, not asserted; the true
    # closures among the accepted ones are as accurate as the host test's bounds say
    assert 0.0 <= z["precision"] <= 1.0 and 0 <= z["true_accepted"] <= z["accept"].sum()
    assert z["recall_ranked"].shape == (4,) and (0 <= z["recall_ranked"]).all() and (z["recall_ranked"] <= 1).all()
    assert 0 <= z["median_yaw_deg"] <= 0.5 and 0 <= z["median_trans_m"] <= 0.2


def test_verify_bench_tool(capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import verify_bench
    rec = verify_bench.main(["--graphs", "120", "--k", "4", "--window", "30", "--reps", "2", "--warmup", "1"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert json.loads(line) == rec
    assert rec["pairs"] == 480 and all(np.isfinite(v) for v in rec.values())
    assert rec["verify_ms"] > 0 and rec["pairs_per_s"] > 0 and rec["hypotheses_max"] >= rec["hypotheses_median"] > 0
