"""sgpr_score_topk off the GPU: host-side argument checks, the workspace bound, recall@N, the sharded AllPairsScorer.topk
(gloo) and the fake kernel of torch.ops.sgpr.score_topk.  CPU only."""
import ctypes
import os

import numpy as np
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


def test_score_topk_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300
    need = lib.sgpr_score_topk_workspace_bytes(h, R, M, 4, 0)
    assert need > 0

    def call(h=h, rows=p, cols=p, vals=p, idx=p, flags=0, k=4, ws=p, ws_bytes=need, r=R):
        return lib.sgpr_score_topk(h, rows, r, cols, M, None, 0, 10, flags, k, vals, idx, ws, ws_bytes, None)

    assert call(h=None) == -1
    assert call(rows=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(cols=None) == -1
    assert call(vals=None) == -1
    assert call(idx=None) == -1
    for k in (0, 17, -3):
        assert call(k=k) == -1 and b"k must" in lib.sgpr_last_error()
    assert call(flags=2) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7
    assert call(r=0, rows=None, cols=None) == 0     # an empty query set needs nothing
    assert lib.sgpr_score_topk_workspace_bytes(h, R, M, 17, 0) == 0
    assert lib.sgpr_score_topk_workspace_bytes(h, R, M, 4, 2) == 0


def test_score_topk_workspace_does_not_grow_with_the_matrix():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    for k in (1, 16):
        n = 20000
        ws = lib.sgpr_score_topk_workspace_bytes(h, n, n, k, 1)
        assert 0 < ws < 0.1 * 4 * n * n
        # twice the rows: the workspace grows with R (operands), not with R * M (the matrix would add 1.6 GB)
        ws2 = lib.sgpr_score_topk_workspace_bytes(h, 2 * n, n, k, 1)
        assert ws2 - ws < 0.01 * 4 * n * n
        big = lib.sgpr_score_topk_workspace_bytes(h, 300000, 300000, k, 0)
        assert 0 < big < 1e9                         # a 300 k-graph map (a 360 GB matrix)


def _brute_recall(idx, xz, p, window, causal):
    m, k = idx.shape
    d = np.sqrt(((xz[:, None, :] - xz[None, :, :]) ** 2).sum(-1))
    hits, counted = np.zeros(k), 0
    for r in range(m):
        ok = [c for c in range(xz.shape[0]) if (window < 0 or abs(c - r) > window) and (not causal or c < r)]
        if not any(d[r, c] <= p for c in ok):
            continue
        counted += 1
        for n in range(1, k + 1):
            if any(j >= 0 and d[r, j] <= p for j in idx[r, :n]):
                hits[n - 1] += 1
    return hits / counted if counted else hits


def test_recall_at_n_against_brute_force():
    from sg_pr_amd import metrics
    rng = np.random.default_rng(4)
    m, k = 120, 5
    xz = np.cumsum(rng.normal(0, 1.0, size=(m, 2)), axis=0)
    xz[80:] = xz[:40] + rng.normal(0, 0.8, size=(40, 2))         # revisits; many queries have none
    idx = rng.integers(-1, m, size=(m, k)).astype(np.int32)
    poses = np.zeros((m, 12))
    poses[:, 3], poses[:, 11] = xz[:, 0], xz[:, 1]
    for window in (-1, 0, 10):
        for causal in (False, True):
            got = metrics.recall_at_n(torch.from_numpy(idx), poses, p_thresh=3.0, window=window, causal=causal, chunk=17)
            want = _brute_recall(idx, xz, 3.0, window, causal)
            assert np.allclose(got, want, rtol=0, atol=1e-12), (window, causal, got, want)
            assert np.all(np.diff(got) >= 0)
    assert np.array_equal(metrics.recall_at_n(torch.full((3, 2), -1, dtype=torch.int32), np.zeros((3, 2)), window=5),
                          np.zeros(2))                                  # no query has a revisit


def _embed(c, l):
    return torch.from_numpy(np.ascontiguousarray(c.reshape(c.shape[0], -1)[:, :32], dtype=np.float32)) * 0.1


def _torch_topk(rows, cols, k=1, window=-1, row0=0, causal=False):
    s = torch.sigmoid((rows.double()[:, None, :] * cols.double()[None, :, :]).sum(-1)).float()   # (no BLAS: same bits on any shard)
    r, m = s.shape
    self_ = torch.arange(r) + row0
    c = torch.arange(m)
    bad = torch.zeros_like(s, dtype=torch.bool)
    if window >= 0:
        bad |= (c[None, :] - self_[:, None]).abs() <= window
    if causal:
        bad |= c[None, :] >= self_[:, None]
    s[bad] = -float("inf")
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    v, i = v[:, :k].contiguous(), i[:, :k].to(torch.int32).contiguous()
    i[v == -float("inf")] = -1
    return v, i


def _graphs():
    from sg_pr_amd import synth
    centers, labels, _, _ = synth.kitti_like_sequence(23, 64, 5)
    return centers, labels


def _topk_worker(rank, world, port, out_dir):
    import sys
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    from sg_pr_amd import allpairs
    torch.set_num_threads(1)
    centers, labels = _graphs()
    sc = allpairs.AllPairsScorer(embed_fn=_embed, score_fn=lambda a, b: a @ b.T, topk_fn=_torch_topk)
    for k, window, causal in ((1, 2, False), (4, 0, True), (3, -1, False)):
        v, i = sc.topk(centers, labels, k=k, window=window, causal=causal)
        torch.save((v, i), os.path.join(out_dir, "w%d_r%d_%d_%d_%d.pt" % (world, rank, k, window, causal)))
    dist.destroy_process_group()


def test_sharded_topk_equals_one_rank(tmp_path):
    from sg_pr_amd import allpairs
    centers, labels = _graphs()
    one = allpairs.AllPairsScorer(embed_fn=_embed, score_fn=lambda a, b: a @ b.T, topk_fn=_torch_topk)
    for world, port in ((2, 29641), (3, 29643)):                  # 23 graphs: 12 + 11 / 8 + 8 + 7 rows
        mp.spawn(_topk_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
        for k, window, causal in ((1, 2, False), (4, 0, True), (3, -1, False)):
            want = one.topk(centers, labels, k=k, window=window, causal=causal)
            assert want[0].shape == (23, k) and want[0].dtype == torch.float32 and want[1].dtype == torch.int32
            for rank in range(world):
                got = torch.load(str(tmp_path / ("w%d_r%d_%d_%d_%d.pt" % (world, rank, k, window, causal))))
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (world, rank, k, window, causal)


def test_score_topk_op_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from sg_pr_amd import ops  # noqa: F401  (registers torch.ops.sgpr.*)
    with FakeTensorMode():
        rows, cols = torch.empty(7, 32, device="cuda"), torch.empty(11, 32, device="cuda")
        blob = torch.empty(48689, device="cuda")
        v, i = torch.ops.sgpr.score_topk(rows, cols, blob, 5, 10, 0, True, None)
        assert v.shape == (7, 5) and v.dtype == torch.float32
        assert i.shape == (7, 5) and i.dtype == torch.int32
        v, i = torch.ops.sgpr.score_topk(rows, cols, blob)
        assert v.shape == (7, 1) and i.shape == (7, 1)
