"""sgpr_topk_rows_large / sgpr_score_topk_large off the GPU: host-side argument checks, the workspace bounds and
metrics.recall_at_percent.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


def test_score_topk_large_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300
    need = lib.sgpr_score_topk_large_workspace_bytes(h, R, M, 100, 0)
    assert need > 0

    def call(h=h, rows=p, cols=p, vals=p, idx=p, flags=0, k=100, ws=p, ws_bytes=need, r=R, row0=0):
        return lib.sgpr_score_topk_large(h, rows, r, cols, M, None, row0, 10, flags, k, vals, idx, ws, ws_bytes, None)

    assert call(h=None) == -1
    assert call(rows=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(cols=None) == -1
    assert call(vals=None) == -1
    assert call(idx=None) == -1
    for k in (0, 4097, -3):
        assert call(k=k) == -1 and b"k must" in lib.sgpr_last_error()
        assert lib.sgpr_score_topk_large_workspace_bytes(h, R, M, k, 0) == 0
    assert call(flags=2) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert lib.sgpr_score_topk_large_workspace_bytes(h, R, M, 100, 2) == 0
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7
    assert call(r=0, rows=None, cols=None) == 0      # an empty query set needs nothing
    assert lib.sgpr_score_topk_large_workspace_bytes(None, R, M, 100, 0) == 0


def test_topk_rows_large_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)
    R, M = 100, 300
    need = lib.sgpr_topk_rows_large_workspace_bytes(h, R, M, 45, 0)
    assert need > 0

    def call(h=h, score=p, vals=p, idx=p, flags=0, k=45, ws=p, ws_bytes=need, r=R, ld=M, window=10, row0=0):
        return lib.sgpr_topk_rows_large(h, score, r, M, ld, None, row0, window, flags, k, vals, idx, ws, ws_bytes, None)

    assert call(h=None) == -1
    assert call(score=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(vals=None) == -1
    assert call(idx=None) == -1
    assert call(ld=M - 1) == -1                      # sgpr_topk_rows' rules: ld >= M, window >= -1
    assert call(window=-2) == -1
    for k in (0, 4097, -3):
        assert call(k=k) == -1 and b"k must" in lib.sgpr_last_error()
        assert lib.sgpr_topk_rows_large_workspace_bytes(h, R, M, k, 0) == 0
    assert call(flags=2) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert lib.sgpr_topk_rows_large_workspace_bytes(h, R, M, 45, 4) == 0
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7
    assert call(r=0) == 0


def test_large_workspaces_do_not_grow_with_the_matrix():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    for fn in (lib.sgpr_score_topk_large_workspace_bytes, lib.sgpr_topk_rows_large_workspace_bytes):
        big = fn(h, 300000, 300000, 4096, 0)
        assert 0 < big < 1e9                          # a 300 k-graph map (a 360 GB matrix)
        for n in (20000, 100000):
            ws, ws2 = fn(h, n, n, 1000, 1), fn(h, 2 * n, n, 1000, 1)
            assert 0 < ws < 0.1 * 4 * n * n
            assert ws2 - ws < 0.01 * 4 * n * n        # doubling R adds far less than the R x M matrix would
        one = fn(h, 1, 1 << 20, 4096, 1)              # one query against a 1 M-frame map: terms linear in M alone
        assert 0 < one < (64 << 20) + 256 * (1 << 20)


def test_recall_percent_n_rounding():
    from sg_pr_amd import metrics
    assert metrics.recall_percent_n(4541) == 45       # KITTI-00
    assert metrics.recall_percent_n(100000) == 1000
    assert metrics.recall_percent_n(10) == 1          # round(0.1) = 0 -> at least one
    assert metrics.recall_percent_n(149) == 1 and metrics.recall_percent_n(151) == 2
    assert metrics.recall_percent_n(1000, 2.5) == 25


def _poses(xz):
    p = np.zeros((xz.shape[0], 12))
    p[:, 3], p[:, 11] = xz[:, 0], xz[:, 1]
    return p


def test_recall_at_percent_by_hand():
    from sg_pr_amd import metrics
    # 300 frames on a line 10 m apart, frames 200..299 revisit frames 0..99 (1 m off): N = 3 at 1 %
    xz = np.zeros((300, 2))
    xz[:, 0] = np.arange(300) * 10.0
    xz[200:, 0] = xz[:100, 0]
    xz[200:, 1] = 1.0
    m = xz.shape[0]
    idx = np.full((m, 4), -1, dtype=np.int32)
    for r in range(200, 300):
        true = r - 200
        slot = {0: 0, 1: 2, 2: 3}[r % 3]                # the revisit at slot 0, 2 or 3 (3: past N)
        row = [(true + 7 + j) % 200 for j in range(4)]
        row[slot] = true
        idx[r] = row
    idx[0] = [200, 1, 2, 3]                           # frame 0 finds its revisit 200 (no window) - a future frame
    rec, n = metrics.recall_at_percent(torch.from_numpy(idx), _poses(xz), percent=1.0, p_thresh=3.0, window=50)
    assert n == 3
    # counted queries: 0..99 (their revisit lies > 50 frames ahead) and 200..299; hits within 3: frame 0 plus the
    # rows with the revisit at slot 0 or 2
    hits = 1 + sum(1 for r in range(200, 300) if r % 3 in (0, 1))
    assert rec == pytest.approx(hits / 200.0, abs=1e-12)
    want = metrics.recall_at_n(torch.from_numpy(idx[:, :3]), _poses(xz), p_thresh=3.0, window=50)[2]
    assert rec == want
    # causal: only frames 200..299 count (a frame may match earlier frames only); frame 0's future hit no longer counts
    rec_c, n_c = metrics.recall_at_percent(torch.from_numpy(idx), _poses(xz), percent=1.0, window=50, causal=True)
    assert n_c == 3 and rec_c == pytest.approx((hits - 1) / 100.0, abs=1e-12)
    # a window wider than the revisit gap: no query counts -> 0
    rec_w, _ = metrics.recall_at_percent(torch.from_numpy(idx), _poses(xz), percent=1.0, window=250)
    assert rec_w == 0.0
    # 2 %: N = 6 but only 4 columns -> ValueError
    with pytest.raises(ValueError, match="6 candidates"):
        metrics.recall_at_percent(torch.from_numpy(idx), _poses(xz), percent=2.0)
    # [M', 2] poses give the same answer as [M', 12] rows
    assert metrics.recall_at_percent(idx, xz, percent=1.0, window=50) == (rec, n)
