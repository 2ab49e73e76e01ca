"""sgpr_score_positives / sgpr_score_threshold_counts: F1-max and ROC area of a whole sequence without the similarity
matrix (fused counting epilogues of the all-pairs tail), on every handle kind, and the layers above them (metrics,
sharded scorer, graph_store and its CLI, two ranks) - every result against the same handle's matrix path, integers and
doubles compared with ==."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(ckpt_path):
    from sg_pr_amd import engine
    from oracle import sgpr_oracle
    e = engine.Engine(sgpr_oracle.load_checkpoint(ckpt_path), device=0)
    yield e
    e.close()


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
def kitti(eng):
    from sg_pr_amd import allpairs, synth
    centers, labels, _, poses = synth.kitti_like_sequence(4541, 100, seed=3)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    return pooled, allpairs.pose_xz(poses).cuda()


def _pooled(n, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 32, generator=g) * scale).cuda()


def _positives_equal(e, rows, cols, row0=0, xz=None, gt=None, what=""):
    score = e.score_all_pairs(rows, cols)
    want, wbad = e.pair_positives(score, row0=row0, pose_xz=xz, gt=gt)
    got, gbad = e.score_positives(rows, cols, row0=row0, pose_xz=xz, gt=gt)
    assert gbad == wbad, what
    assert torch.equal(torch.sort(got.view(torch.int32))[0], torch.sort(want.view(torch.int32))[0]), what
    return score, want


def _rank_of(pos, t):
    from sg_pr_amd import metrics
    u, mult = metrics.distinct_counts(pos.cpu().numpy())
    above = np.concatenate((np.cumsum(mult[::-1])[::-1], [0])).astype(np.int64)
    step = max(1, -(-u.size // t))
    return u[::step], (u, step, above)


def _counts_equal(e, rows, cols, score, thr, row0=0, xz=None, gt=None, rank=None, what=""):
    want = e.pair_threshold_counts(score, thr, row0=row0, pose_xz=xz, gt=gt, rank=rank)
    got = e.score_threshold_counts(rows, cols, thr, row0=row0, pose_xz=xz, gt=gt, rank=rank)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], what


def test_kitti_positives_counts_and_metrics(eng, kitti):
    from sg_pr_amd import metrics
    pooled, xz = kitti
    score, pos = _positives_equal(eng, pooled, pooled, xz=xz, what="kitti")
    assert pos.numel() > 1000
    cap = eng.MAX_POOLED_THRESHOLDS
    assert cap == 2047
    for t in (1, 7, cap):
        thr, rank = _rank_of(pos, t)
        assert thr.size <= t
        _counts_equal(eng, pooled, pooled, score, thr, xz=xz, what=("T", t))
        _counts_equal(eng, pooled, pooled, score, thr, xz=xz, rank=rank, what=("T rank", t))
    f1, auc, passes = metrics.pr_roc_pooled(eng, pooled, pooled, pose_xz=xz)
    f1m, aucm, passes_m = metrics.pr_roc_device(eng, score, pose_xz=xz)
    print("kitti: F1 %.6f AUC %.6f passes pooled %d matrix %d" % (f1, auc, passes, passes_m))
    assert f1 == f1m and auc == aucm
    assert metrics.f1_max_pooled(eng, pooled, pooled, pose_xz=xz)[0] == float(eng.f1_max(score, pose_xz=xz)[0])
    assert metrics.roc_auc_pooled(eng, pooled, pooled, pose_xz=xz) == aucm


@pytest.mark.parametrize("r,m,row0", [(1, 1, 0), (1, 700, 3), (37, 1, 9), (100, 333, 0), (257, 513, 40), (300, 300, 0)])
def test_rectangles(eng, kitti, r, m, row0):
    pooled, xz = kitti
    rows, cols = pooled[row0:row0 + r].contiguous(), pooled[:m].contiguous()
    score, pos = _positives_equal(eng, rows, cols, row0=row0, xz=xz, what=(r, m, row0))
    for t in (1, 7):
        thr = np.unique(np.quantile(score.cpu().numpy(), np.linspace(0.05, 0.95, t)).astype(np.float32))
        _counts_equal(eng, rows, cols, score, thr, row0=row0, xz=xz, what=(r, m, row0, t))
        if pos.numel():
            thr, rank = _rank_of(pos, t)
            _counts_equal(eng, rows, cols, score, thr, row0=row0, xz=xz, rank=rank, what=(r, m, row0, t, "rank"))


def test_explicit_labels_with_ignored_cells(eng):
    from sg_pr_amd import metrics
    rows, cols = _pooled(150, 1), _pooled(411, 2)
    g = torch.Generator().manual_seed(3)
    gt = (torch.randint(0, 20, (150, 411), generator=g) - 1).clamp(max=1).to(torch.int8)    # -1 / 0 / 1
    gt[gt == 1] = torch.where(torch.rand(int((gt == 1).sum()), generator=g) < 0.2, 1, 0).to(torch.int8)
    score, pos = _positives_equal(eng, rows, cols, gt=gt, what="gt")
    assert pos.numel() > 0
    thr, rank = _rank_of(pos, 7)
    _counts_equal(eng, rows, cols, score, thr, gt=gt, rank=rank, what="gt")
    got = metrics.pr_roc_pooled(eng, rows, cols, gt=gt)
    want = metrics.pr_roc_device(eng, score, gt=gt)
    assert got[:2] == want[:2]


def test_no_positives(eng, kitti):
    from sg_pr_amd import metrics
    pooled, xz = kitti
    far = xz.clone()
    far[:, 0] += torch.arange(far.shape[0], device=far.device, dtype=torch.float64) * 100.0   # frames 100 m apart
    rows, cols = pooled[300:500], pooled[:300]                                  # no frame meets itself
    f1, auc, passes = metrics.pr_roc_pooled(eng, rows, cols, pose_xz=far, row0=300)
    assert f1 == 0.0 and np.isnan(auc) and passes == 0
    got, bad = eng.score_positives(rows, cols, pose_xz=far, row0=300)
    assert got.numel() == 0 and bad == 0


def test_negative_and_nan_scores(eng, kitti):
    """Pooled vectors with NaN / infinite entries: positives, skipped counts and bucket counts equal the matrix path's,
    and the metrics raise ValueError exactly when the matrix path does (a sigmoid score is never negative; a NaN one
    is skipped and reported)."""
    from sg_pr_amd import metrics
    pooled, xz = kitti
    thr = np.array([0.2, 0.5, 0.9], dtype=np.float32)
    for what, v in (("nan", float("nan")), ("inf", float("inf")), ("-inf", float("-inf"))):
        rows, cols = pooled[:64].clone(), pooled[:500].clone()
        rows[3, ::2] = v
        rows[3, 1::2] = -v
        cols[7] = v
        score, _ = _positives_equal(eng, rows, cols, xz=xz, what=what)
        _counts_equal(eng, rows, cols, score, thr, xz=xz, what=what)
        try:
            want = metrics.pr_roc_device(eng, score, pose_xz=xz)
        except ValueError:
            want = "raised"
        try:
            got = metrics.pr_roc_pooled(eng, rows, cols, pose_xz=xz)
        except ValueError:
            got = "raised"
        assert (got == "raised") == (want == "raised"), what
        if torch.isnan(score).any():
            assert got == "raised", what
        else:
            assert got[:2] == want[:2], what


def test_fallback_handles(eng, kitti, oracle_sd):
    """Debug bit 13 (three-plane tail), a wide-range checkpoint and an any-shape handle: equal to their own matrix."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import score_ref
    from sg_pr_amd import engine, metrics, sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    pooled, xz = kitti
    rows, cols = pooled[100:400].contiguous(), pooled[:900].contiguous()

    def check(e, r, c, x, row0, what):
        score, pos = _positives_equal(e, r, c, row0=row0, xz=x, what=what)
        thr, rank = _rank_of(pos, 7)
        _counts_equal(e, r, c, score, thr, row0=row0, xz=x, rank=rank, what=what)
        assert metrics.pr_roc_pooled(e, r, c, pose_xz=x, row0=row0)[:2] == \
            metrics.pr_roc_device(e, score, pose_xz=x, row0=row0)[:2], what
    eng.set_skip_mask(1 << 13)
    try:
        check(eng, rows, cols, xz, 100, "bit 13")
    finally:
        eng.set_skip_mask(0)
    wide_sd = score_ref.dead_neuron_with_huge_fold(oracle_sd, [(rows.cpu().numpy(), cols.cpu().numpy())])[0]
    ew = engine.Engine(wide_sd, device=0)
    try:
        check(ew, rows, cols, xz, 100, "wide")
    finally:
        ew.close()
    args = sgpr_args()
    args.filters_1, args.filters_2, args.filters_3, args.tensor_neurons, args.bottle_neck_neurons = 64, 64, 48, 16, 16
    args.node_num, args.K = 64, 10
    torch.manual_seed(5)
    m = sg_net.SG(args, 12).eval()
    e2 = m.engine()
    assert e2.any_shape
    g = torch.Generator().manual_seed(6)
    pr, pc = torch.randn(233, 48, generator=g).cuda(), torch.randn(350, 48, generator=g).cuda()
    check(e2, pr, pc, xz, 17, "any-shape")
    f1, auc, _ = m.evaluate_pooled(pr, pc, pose_xz=xz, row0=17)
    assert (f1, auc) == metrics.pr_roc_device(e2, e2.score_all_pairs(pr, pc), pose_xz=xz, row0=17)[:2]


def test_any_workspace_contents(eng, kitti):
    """0x00 / 0xFF / random workspaces give the same bytes (the call depends on its arguments only)."""
    pooled, xz = kitti
    lib, h = eng.lib, eng._h
    rows, cols = pooled[:700].contiguous(), pooled.contiguous()
    r, m = rows.shape[0], cols.shape[0]
    thr = np.array([0.1, 0.4, 0.7, 0.95], dtype=np.float32)
    dthr = torch.from_numpy(thr).cuda()
    outs = []
    for fill in (0x00, 0xFF, None):
        nb = lib.sgpr_score_threshold_counts_workspace_bytes(h, r, m, 4)
        nbp = lib.sgpr_score_positives_workspace_bytes(h, r, m)
        ws = torch.empty(max(nb, nbp), dtype=torch.uint8, device="cuda")
        if fill is None:
            ws.random_(0, 256)
        else:
            ws.fill_(fill)
        out = torch.full((7,), -1, dtype=torch.int64, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731
        assert lib.sgpr_score_threshold_counts(h, vp(rows), r, vp(cols), m, 0, vp(xz), 3.0, 20.0, None, m, vp(dthr), 4,
                                               None, 0, None, vp(out), vp(ws), ws.numel(), st) == 0
        pos = torch.full((1 << 16,), -1.0, device="cuda")
        cnt = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        if fill is None:
            ws.random_(0, 256)
        assert lib.sgpr_score_positives(h, vp(rows), r, vp(cols), m, 0, vp(xz), 3.0, 20.0, None, m, vp(pos), pos.numel(),
                                        vp(cnt), vp(ws), ws.numel(), st) == 0
        n = int(cnt[0])
        outs.append((out.cpu(), cnt.cpu(), torch.sort(pos[:n].view(torch.int32))[0].cpu()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def test_invalid_arguments(eng, kitti):
    from sg_pr_amd import engine
    pooled, xz = kitti
    lib, h = eng.lib, eng._h
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                                         # noqa: E731
    rows, cols = pooled[:20], pooled[:40]
    out = torch.zeros(2100, dtype=torch.int64, device="cuda")
    thr = torch.linspace(0, 1, 2048, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    INV, WS = -1, -7
    assert engine.ERROR_NAMES[WS] == "SGPR_E_WORKSPACE"

    def tc(**kw):
        a = dict(h=h, rows=vp(rows), R=20, cols=vp(cols), M=40, row0=0, pose=vp(xz), gt=None, ldg=40, thr=vp(thr), T=7,
                 rank=None, gpt=0, atl=None, out=vp(out), ws=vp(ws), wsb=ws.numel())
        a.update(kw)
        return lib.sgpr_score_threshold_counts(a["h"], a["rows"], a["R"], a["cols"], a["M"], a["row0"], a["pose"], 3.0,
                                               20.0, a["gt"], a["ldg"], a["thr"], a["T"], a["rank"], a["gpt"], a["atl"],
                                               a["out"], a["ws"], a["wsb"], None)

    def pc(**kw):
        a = dict(h=h, rows=vp(rows), R=20, cols=vp(cols), M=40, row0=0, pose=vp(xz), gt=None, ldg=40, out=None, cap=0,
                 cnt=vp(cnt), ws=vp(ws), wsb=ws.numel())
        a.update(kw)
        return lib.sgpr_score_positives(a["h"], a["rows"], a["R"], a["cols"], a["M"], a["row0"], a["pose"], 3.0, 20.0,
                                        a["gt"], a["ldg"], a["out"], a["cap"], a["cnt"], a["ws"], a["wsb"], None)
    assert tc() == 0 and pc() == 0
    torch.cuda.synchronize()
    assert tc(T=2047) == 0
    for bad in (dict(h=None), dict(R=-1), dict(M=-1), dict(rows=None), dict(cols=None), dict(pose=None), dict(out=None),
                dict(T=-1), dict(T=2048), dict(thr=None), dict(rank=vp(thr)), dict(row0=0x7fffffff)):
        assert tc(**bad) == INV, bad
    for bad in (dict(h=None), dict(R=-1), dict(M=-1), dict(rows=None), dict(pose=None), dict(cnt=None), dict(cap=-1),
                dict(cap=5)):
        assert pc(**bad) == INV, bad
    assert tc(ws=None) == WS and tc(wsb=16) == WS
    assert pc(ws=None) == WS and pc(wsb=16) == WS
    with pytest.raises(engine.SgprError):
        eng.score_threshold_counts(rows, cols, np.linspace(0, 1, 2048), pose_xz=xz)


def test_scale_30k_and_workspace_bounds(eng, kitti):
    """R = M = 30 000 (a 3.6 GB matrix) equals the row-blocked matrix path; the workspaces (the tail's operands, 2 KB per
    row) stay below 128 MB there and below 1 GB at 300 000 (a 360 GB matrix)."""
    pooled, xz = kitti
    reps = -(-30000 // pooled.shape[0])
    big = pooled.repeat(reps, 1)[:30000].contiguous()
    bxz = torch.cat([xz + torch.tensor([i * 1000.0, 0.0], device=xz.device, dtype=xz.dtype) for i in range(reps)])[:30000]
    bxz = bxz.contiguous()
    t = 2047
    assert eng.score_threshold_counts_workspace_bytes(30000, 30000, t) < 128 << 20
    assert eng.score_positives_workspace_bytes(30000, 30000) < 128 << 20
    assert eng.score_threshold_counts_workspace_bytes(300000, 300000, t) < 1 << 30
    assert eng.score_positives_workspace_bytes(300000, 300000) < 1 << 30
    pos_parts, bad_parts, blocks = [], 0, []
    for r0 in range(0, 30000, 4096):
        score = eng.score_all_pairs(big[r0:r0 + 4096], big)
        p, b = eng.pair_positives(score, row0=r0, pose_xz=bxz)
        pos_parts.append(p)
        bad_parts += b
        blocks.append((r0, score))
    want_pos = torch.cat(pos_parts)
    got_pos, got_bad = eng.score_positives(big, big, pose_xz=bxz)
    assert got_bad == bad_parts
    assert torch.equal(torch.sort(got_pos.view(torch.int32))[0], torch.sort(want_pos.view(torch.int32))[0])
    thr, rank = _rank_of(want_pos, t)
    want = [np.zeros(thr.size + 1, dtype=np.int64), 0, 0]
    for r0, score in blocks:
        c, b, rs = eng.pair_threshold_counts(score, thr, row0=r0, pose_xz=bxz, rank=rank)
        want[0] += c
        want[1] += b
        want[2] += rs
    del blocks, score
    got = eng.score_threshold_counts(big, big, thr, pose_xz=bxz, rank=rank)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]


def test_scorer_and_graph_store(model, tmp_path, ckpt_path):
    from sg_pr_amd import allpairs, graph_store, synth
    centers, labels, _, poses = synth.kitti_like_sequence(700, 100, seed=12)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(700)])
    a = graph_store.evaluate_all_pairs(model, seq, top_k=4)
    b = graph_store.evaluate_all_pairs(model, seq, top_k=4, keep_matrix=False)
    assert b["matrix"] is None and a["matrix"] is not None
    assert a["f1_max"] == b["f1_max"] and (a["roc_auc"] == b["roc_auc"] or (np.isnan(a["roc_auc"]) and np.isnan(b["roc_auc"])))
    assert a["f1_max"] > 0
    assert torch.equal(a["closure_scores"], b["closure_scores"]) and torch.equal(a["closure_frames"], b["closure_frames"])
    scorer = allpairs.AllPairsScorer(model=model)
    f1, auc = scorer.pr_roc_pooled(centers, labels, poses)
    assert (f1, auc) == (a["f1_max"], a["roc_auc"])
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
    r1 = graph_store.main([str(cfg)])
    f_matrix = (tmp_path / "eva" / "07_allpairs_F1_max.txt").read_text()
    c_matrix = np.load(tmp_path / "eva" / "07_loop_closures.npy")
    r2 = graph_store.main([str(cfg), "--no-matrix"])
    assert (tmp_path / "eva" / "07_allpairs_F1_max.txt").read_text() == f_matrix and r1 == r2
    assert np.array_equal(np.load(tmp_path / "eva" / "07_loop_closures.npy"), c_matrix)


def _two_rank_worker(rank, world, port, ckpt, out_dir):
    import sys
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sg_pr_amd import allpairs, sg_net, synth
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt
    trainer = sg_net.SGTrainer(args, False)
    centers, labels, _, poses = synth.kitti_like_sequence(403, 100, 6)              # 202 + 201 rows: uneven shards
    dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
    scorer = allpairs.AllPairsScorer(model=trainer.model)
    got = scorer.pr_roc_pooled(dc, dl, poses)
    if rank == 1:
        torch.save(torch.tensor(got, dtype=torch.float64), os.path.join(out_dir, "pr_roc.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path, ckpt_path, model):
    import torch.multiprocessing as mp
    from sg_pr_amd import allpairs, synth
    mp.spawn(_two_rank_worker, args=(2, 29671, ckpt_path, str(tmp_path)), nprocs=2, join=True)
    centers, labels, _, poses = synth.kitti_like_sequence(403, 100, 6)
    scorer = allpairs.AllPairsScorer(model=model)
    one = scorer.pr_roc_pooled(torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda(), poses)
    two = torch.load(str(tmp_path / "pr_roc.pt"))
    assert one[0] > 0
    assert one[0] == float(two[0]) and (one[1] == float(two[1]) or (np.isnan(one[1]) and np.isnan(float(two[1]))))
