"""sgpr_score_above / sgpr_rows_above off the GPU: host-side argument checks, the workspace bound, precision / recall at
a threshold, the sharded AllPairsScorer.above (gloo) and the fake kernel of torch.ops.sgpr.score_above.  CPU only."""
import ctypes
import os

import numpy as np
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


def test_score_above_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300
    need = lib.sgpr_score_above_workspace_bytes(h, R, M, 0)
    assert need > 0

    def call(h=h, rows=p, cols=p, o_r=p, o_c=p, o_v=p, cap=1000, rp=p, count=p, flags=0, thr=0.5, ws=p,
             ws_bytes=need, r=R, row0=0):
        return lib.sgpr_score_above(h, rows, r, cols, M, None, row0, 10, flags, thr, o_r, o_c, o_v, cap, rp, count, ws,
                                    ws_bytes, None)

    assert call(h=None) == -1
    assert call(rows=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(cols=None) == -1
    for kw in ("o_r", "o_c", "o_v"):
        assert call(**{kw: None}) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(count=None) == -1
    assert call(cap=-1) == -1 and b"capacity" in lib.sgpr_last_error()
    assert call(r=-1) == -1
    assert call(flags=2) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert call(thr=float("nan")) == -1 and b"NaN" in lib.sgpr_last_error()
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7
    assert lib.sgpr_score_above_workspace_bytes(h, R, M, 2) == 0
    assert lib.sgpr_score_above_workspace_bytes(h, R, 0, 0) == 0

    need_r = lib.sgpr_rows_above_workspace_bytes(h, R, M)
    assert need_r > 0

    def rcall(score=p, ld=M, o_r=p, o_c=p, o_v=p, cap=1000, count=p, flags=0, thr=0.5, ws=p, ws_bytes=need_r):
        return lib.sgpr_rows_above(h, score, R, M, ld, None, 0, 10, flags, thr, o_r, o_c, o_v, cap, None, count, ws,
                                   ws_bytes, None)

    assert rcall(score=None) == -1
    assert rcall(ld=M - 1) == -1
    assert rcall(o_v=None) == -1
    assert rcall(cap=-5) == -1
    assert rcall(count=None) == -1
    assert rcall(flags=4) == -1
    assert rcall(thr=float("nan")) == -1
    assert rcall(ws_bytes=need_r - 1) == -7
    assert lib.sgpr_rows_above_workspace_bytes(h, R, 0) == 0


def test_score_above_workspace_does_not_grow_with_the_matrix():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    n = 20000
    for flags in (0, 1):
        ws = lib.sgpr_score_above_workspace_bytes(h, n, n, flags)
        assert 0 < ws < 0.1 * 4 * n * n
        ws2 = lib.sgpr_score_above_workspace_bytes(h, 2 * n, n, flags)
        assert ws2 - ws < 0.01 * 4 * n * n           # grows with R, not with R * M (the matrix would add 1.6 GB)
        big = lib.sgpr_score_above_workspace_bytes(h, 300000, 300000, flags)
        assert 0 < big < 1e9                         # a 300 k-graph map (a 360 GB matrix)
    assert 0 < lib.sgpr_rows_above_workspace_bytes(h, 300000, 300000) < 1e7   # O(R)


def _brute_pr(rows, cols, xz, p, n, window, causal):
    d = np.sqrt(((xz[:, None, :] - xz[None, :, :]) ** 2).sum(-1))
    m = xz.shape[0]
    tp = sum(1 for r, c in zip(rows, cols) if d[r, c] <= p)
    fp = sum(1 for r, c in zip(rows, cols) if d[r, c] >= n)
    pos = 0
    for r in range(m):
        for c in range(m):
            if (window < 0 or abs(c - r) > window) and (not causal or c < r) and d[r, c] <= p:
                pos += 1
    return (tp / (tp + fp) if tp + fp else 0.0), (tp / pos if pos else 0.0)


def test_precision_recall_at_against_brute_force():
    from sg_pr_amd import metrics
    rng = np.random.default_rng(8)
    m = 90
    xz = np.cumsum(rng.normal(0, 1.5, size=(m, 2)), axis=0)
    xz[60:] = xz[:30] + rng.normal(0, 1.0, size=(30, 2))         # revisits
    poses = np.zeros((m, 12))
    poses[:, 3], poses[:, 11] = xz[:, 0], xz[:, 1]
    pairs = rng.integers(0, m, size=(400, 2))
    for window in (-1, 0, 10):
        for causal in (False, True):
            ok = [(r, c) for r, c in pairs if (window < 0 or abs(c - r) > window) and (not causal or c < r)]
            rows = np.array([r for r, _ in ok], dtype=np.int32)
            cols = np.array([c for _, c in ok], dtype=np.int32)
            got = metrics.precision_recall_at(torch.from_numpy(rows), torch.from_numpy(cols), poses, p_thresh=3.0,
                                              n_thresh=20.0, window=window, causal=causal, chunk=7)
            want = _brute_pr(rows, cols, xz, 3.0, 20.0, window, causal)
            assert abs(got[0] - want[0]) < 1e-12 and abs(got[1] - want[1]) < 1e-12, (window, causal, got, want)
    empty = torch.zeros(0, dtype=torch.int32)
    assert metrics.precision_recall_at(empty, empty, poses) == (0.0, 0.0)


def _embed(c, l):
    return torch.from_numpy(np.ascontiguousarray(c.reshape(c.shape[0], -1)[:, :32], dtype=np.float32)) * 0.1


def _torch_above(rows, cols, threshold, window=-1, row0=0, causal=False):
    s = torch.sigmoid((rows.double()[:, None, :] * cols.double()[None, :, :]).sum(-1)).float()   # (no BLAS: same bits on any shard)
    r, m = s.shape
    self_ = torch.arange(r) + row0
    c = torch.arange(m)
    ok = s >= threshold
    if window >= 0:
        ok &= (c[None, :] - self_[:, None]).abs() > window
    if causal:
        ok &= c[None, :] < self_[:, None]
    nz = torch.nonzero(ok)
    rp = torch.zeros(r + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(ok.sum(dim=1), 0)
    return nz[:, 0].to(torch.int32), nz[:, 1].to(torch.int32), s[ok], rp


_CASES = ((0.5, 2, False), (0.6, 0, True), (-float("inf"), -1, False), (float("inf"), 3, False))


def _graphs():
    from sg_pr_amd import synth
    centers, labels, _, _ = synth.kitti_like_sequence(23, 64, 5)
    return centers, labels


def _above_worker(rank, world, port, out_dir):
    import sys
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    from sg_pr_amd import allpairs
    torch.set_num_threads(1)
    centers, labels = _graphs()
    sc = allpairs.AllPairsScorer(embed_fn=_embed, score_fn=lambda a, b: a @ b.T, above_fn=_torch_above)
    for j, (thr, window, causal) in enumerate(_CASES):
        got = sc.above(centers, labels, thr, window=window, causal=causal)
        torch.save(got, os.path.join(out_dir, "w%d_r%d_%d.pt" % (world, rank, j)))
    dist.destroy_process_group()


def test_sharded_above_equals_one_rank(tmp_path):
    from sg_pr_amd import allpairs
    centers, labels = _graphs()
    one = allpairs.AllPairsScorer(embed_fn=_embed, score_fn=lambda a, b: a @ b.T, above_fn=_torch_above)
    wants = [one.above(centers, labels, thr, window=window, causal=causal) for thr, window, causal in _CASES]
    assert wants[2][0].numel() == 23 * 23 and wants[3][0].numel() == 0
    assert wants[0][0].numel() > 0 and wants[0][3][-1] == wants[0][0].numel()
    for world, port in ((2, 29651), (3, 29653)):                  # 23 graphs: 12 + 11 / 8 + 8 + 7 rows
        mp.spawn(_above_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
        for j, want in enumerate(wants):
            for rank in range(world):
                got = torch.load(str(tmp_path / ("w%d_r%d_%d.pt" % (world, rank, j))))
                assert len(got) == 4
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and torch.equal(g, w), (world, rank, j)


def test_score_above_op_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    from sg_pr_amd import ops  # noqa: F401  (registers torch.ops.sgpr.*)
    with FakeTensorMode(shape_env=ShapeEnv()):
        rows, cols = torch.empty(7, 32, device="cuda"), torch.empty(11, 32, device="cuda")
        blob = torch.empty(48689, device="cuda")
        r, c, v, rp = torch.ops.sgpr.score_above(rows, cols, blob, 0.5, 10, 0, True, None, None)
        assert r.dtype == torch.int32 and c.dtype == torch.int32 and v.dtype == torch.float32
        assert rp.shape == (8,) and rp.dtype == torch.int64
        assert isinstance(r.shape[0], torch.SymInt) and r.shape == c.shape == v.shape     # a data-dependent length
        r, c, v, rp = torch.ops.sgpr.score_above(rows, cols, blob, 0.5, capacity=40)
        assert r.shape == (40,) and v.shape == (40,) and rp.shape == (8,)
