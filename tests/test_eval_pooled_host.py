"""sgpr_score_positives / sgpr_score_threshold_counts off the GPU: the symbols and the ABI version, host-side argument
checks, the workspace bounds, and metrics.pr_roc_pooled's orchestration with numpy stand-in producers.  CPU only."""
import ctypes
import re
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


def test_symbols_and_abi_version():
    from sg_pr_amd import engine
    lib = engine.load_library()
    for name in ("sgpr_score_positives", "sgpr_score_positives_workspace_bytes", "sgpr_score_threshold_counts",
                 "sgpr_score_threshold_counts_workspace_bytes"):
        assert name in engine.ABI_SYMBOLS
        assert hasattr(lib, name)
    assert lib.sgpr_abi_version() == 11
    with open(os.path.join(REPO, "include", "sgpr.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+SGPR_SCORE_COUNT_MAX_THRESHOLDS\s+(\d+)", header).group(1)) == \
        engine.Engine.MAX_POOLED_THRESHOLDS


def test_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300
    need_c = lib.sgpr_score_threshold_counts_workspace_bytes(h, R, M, 7)
    need_p = lib.sgpr_score_positives_workspace_bytes(h, R, M)
    assert need_c > 0 and need_p > 0

    def counts(h=h, rows=p, cols=p, r=R, row0=0, pose=p, gt=None, ldg=M, thr=p, t=7, rank=None, gpt=0, atl=None, out=p,
               ws=p, ws_bytes=need_c):
        return lib.sgpr_score_threshold_counts(h, rows, r, cols, M, row0, pose, 3.0, 20.0, gt, ldg, thr, t, rank, gpt,
                                               atl, out, ws, ws_bytes, None)

    def positives(h=h, rows=p, cols=p, r=R, row0=0, pose=p, gt=None, ldg=M, out=p, cap=10, count=p, ws=p,
                  ws_bytes=need_p):
        return lib.sgpr_score_positives(h, rows, r, cols, M, row0, pose, 3.0, 20.0, gt, ldg, out, cap, count, ws,
                                        ws_bytes, None)

    for call in (counts, positives):
        assert call(h=None) == -1
        assert call(rows=None) == -1
        assert call(cols=None) == -1
        assert call(r=-1) == -1
        assert call(pose=None) == -1                                  # no ground truth at all
        assert call(pose=None, gt=p, ldg=M - 1) == -1                 # labels narrower than the rectangle
        assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
        assert call(ws=None) == -7 and b"workspace" in lib.sgpr_last_error()
        assert call(ws_bytes=16) == -7
    assert counts(out=None) == -1
    assert counts(t=-1) == -1
    assert counts(t=2048) == -1 and b"2047" in lib.sgpr_last_error()
    assert counts(thr=None) == -1
    assert counts(rank=p, gpt=0, atl=p) == -1 and b"ranking" in lib.sgpr_last_error()
    assert counts(rank=p, gpt=1, atl=None) == -1
    assert positives(count=None) == -1
    assert positives(cap=-1) == -1
    assert positives(out=None) == -1
    assert lib.sgpr_score_threshold_counts_workspace_bytes(h, R, M, 2048) == 0
    assert lib.sgpr_score_threshold_counts_workspace_bytes(h, R, 0, 7) == 0
    assert lib.sgpr_score_positives_workspace_bytes(h, -1, M) == 0


def test_workspace_grows_with_rows_and_columns_not_pairs():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    lib.sgpr_score_threshold_counts_workspace_bytes.restype = ctypes.c_size_t
    big = lib.sgpr_score_threshold_counts_workspace_bytes(h, 300000, 300000, 2047)
    assert 0 < big < 1 << 30                                          # the matrix would be 360 GB
    assert 0 < lib.sgpr_score_positives_workspace_bytes(h, 300000, 300000) < 1 << 30
    a = lib.sgpr_score_threshold_counts_workspace_bytes(h, 100000, 100000, 2047)
    b = lib.sgpr_score_threshold_counts_workspace_bytes(h, 200000, 200000, 2047)
    assert b < 2.5 * a                                                # linear, not quadratic


class _NumpyEngine:
    """metrics.counts_of as the producers of score_positives / score_threshold_counts (pooled vectors are stand-in
    indices into a host score matrix)."""
    MAX_POOLED_THRESHOLDS = 5

    def __init__(self, score, gt):
        self.score, self.gt = score, gt
        self.calls = []

    def _sub(self, rows, cols):
        r, c = np.asarray(rows).ravel(), np.asarray(cols).ravel()
        return self.score[np.ix_(r, c)], self.gt[np.ix_(r, c)]

    def score_positives(self, rows, cols, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0, gt=None):
        from sg_pr_amd import metrics
        s, g = self._sub(rows, cols)
        pos, _ = metrics.counts_of(s, g)
        return torch.from_numpy(np.ascontiguousarray(pos)), 0

    def score_threshold_counts(self, rows, cols, thresholds, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0, gt=None,
                               rank=None):
        from sg_pr_amd import metrics
        assert len(thresholds) <= self.MAX_POOLED_THRESHOLDS
        self.calls.append(len(thresholds))
        s, g = self._sub(rows, cols)
        counts, rank_sum = metrics.counts_of(s, g)[1](thresholds, rank)
        return counts, 0, rank_sum


def test_pr_roc_pooled_orchestration_equals_host_metrics():
    from sg_pr_amd import metrics
    rng = np.random.default_rng(4)
    for trial in range(6):
        r, m = 40 + trial, 60
        score = np.round(rng.random((r, m)), 2).astype(np.float32)          # ties on purpose
        gt = rng.choice([-1, 0, 1], size=(r, m), p=[0.1, 0.75, 0.15]).astype(np.int8)
        gt[score > 0.8] = np.where(rng.random(int((score > 0.8).sum())) < 0.6, 1, gt[score > 0.8])
        e = _NumpyEngine(score, gt)
        rows, cols = np.arange(r), np.arange(m)
        f1, auc, passes = metrics.pr_roc_pooled(e, rows, cols, gt=gt)
        keep = gt.ravel() >= 0
        assert abs(f1 - metrics.f1_max(gt.ravel()[keep], score.ravel()[keep])) < 1e-12
        assert abs(auc - metrics.roc_auc(gt.ravel()[keep], score.ravel()[keep])) < 1e-12
        assert passes >= 1 and max(e.calls) <= 5
        assert metrics.f1_max_pooled(e, rows, cols, gt=gt)[0] == f1
        assert metrics.roc_auc_pooled(e, rows, cols, gt=gt) == auc
    e = _NumpyEngine(np.full((3, 3), 0.5, np.float32), np.zeros((3, 3), np.int8))
    f1, auc, passes = metrics.pr_roc_pooled(e, np.arange(3), np.arange(3), gt=e.gt)
    assert f1 == 0.0 and np.isnan(auc) and passes == 0


def test_sharded_pr_roc_pooled_routes_through_pr_roc():
    """One rank: AllPairsScorer.pr_roc_pooled = pr_roc over the pooled producers with the engine's threshold cap."""
    from sg_pr_amd import allpairs, metrics
    rng = np.random.default_rng(9)
    m = 50
    score = rng.random((m, m)).astype(np.float32)
    poses = np.zeros((m, 2))
    poses[:, 0] = np.arange(m) * 2.0
    d = np.abs(poses[:, None, 0] - poses[None, :, 0])
    gt = np.where(d <= 3.0, 1, np.where(d >= 20.0, 0, -1)).astype(np.int8)
    e = _NumpyEngine(score, gt)

    def embed(c, l):
        return torch.as_tensor(np.asarray(c)).view(-1, 1)

    scorer = allpairs.AllPairsScorer(embed_fn=embed, score_fn=lambda a, b: None)
    f1, auc = scorer.pr_roc_pooled(np.arange(m), np.zeros((m, 1)), poses, engine=e)
    keep = gt.ravel() >= 0
    assert abs(f1 - metrics.f1_max(gt.ravel()[keep], score.ravel()[keep])) < 1e-12
    assert abs(auc - metrics.roc_auc(gt.ravel()[keep], score.ravel()[keep])) < 1e-12
    assert max(e.calls) <= 5
