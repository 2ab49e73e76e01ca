#!/usr/bin/env python3
"""Whole-sequence evaluation timings: F1-max + ROC area without the matrix (sgpr_score_positives +
sgpr_score_threshold_counts, metrics.pr_roc_pooled) against score_all_pairs + metrics.pr_roc_device (row-blocked
beyond 64 M entries).

    python tools/run_eval_pooled.py [--reps 5] [--only kitti|100k]

One JSON line per case: KITTI-00 (4541 x 4541, the synthetic KITTI-like sequence, shipped checkpoint) and a 100 000-graph
set (the KITTI-like pooled vectors and poses repeated, each copy 1 km away from the others).  Per case: the median wall
time of each whole path (CUDA events, inputs resident), its counting passes, the threshold cap of each path, the peak
device memory each path adds, whether F1 and the area agree exactly, and - KITTI-00 only - the median time of one
positives call and of one counting call at the cap with ranking.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], out


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def matrix_path(eng, pooled, xz):
    """score_all_pairs + pr_roc_device, in row blocks of at most 64 M entries (the whole matrix when it fits); the
    blocks' positives are gathered and their counts summed, like AllPairsScorer.pr_roc does across ranks"""
    from sg_pr_amd import metrics
    m = pooled.shape[0]
    rb = max(1, min(m, (64 << 20) // m))
    if rb == m:
        return metrics.pr_roc_device(eng, eng.score_all_pairs(pooled, pooled), pose_xz=xz)
    buf = torch.empty(rb, m, dtype=torch.float32, device=pooled.device)
    blocks = [(r0, min(rb, m - r0)) for r0 in range(0, m, rb)]
    pos = []
    for r0, n in blocks:
        eng.score_all_pairs(pooled[r0:r0 + n], pooled, out=buf[:n])
        pos.append(eng.pair_positives(buf[:n], row0=r0, pose_xz=xz)[0])

    def count_fn(thr, rank):
        tot, rs = None, 0
        for r0, n in blocks:
            eng.score_all_pairs(pooled[r0:r0 + n], pooled, out=buf[:n])
            c, _, r = eng.pair_threshold_counts(buf[:n], thr, row0=r0, pose_xz=xz, rank=rank)
            tot = c if tot is None else tot + c
            rs += r or 0
        return tot, (rs if rank is not None else None)
    return metrics.pr_roc_from_counts(torch.cat(pos).cpu().numpy(), count_fn)


def case(eng, name, pooled, xz, reps, calls=False):
    from sg_pr_amd import metrics
    m = pooled.shape[0]
    res = {"case": name, "M": m, "cap_pooled": eng.MAX_POOLED_THRESHOLDS, "cap_matrix": metrics.MAX_THRESHOLDS}
    res["pooled_ms"], (f1, auc, passes) = timed(lambda: metrics.pr_roc_pooled(eng, pooled, pooled, pose_xz=xz), reps)
    res["matrix_ms"], (f1m, aucm, passes_m) = timed(lambda: matrix_path(eng, pooled, xz), reps)
    res.update(passes_pooled=passes, passes_matrix=passes_m, f1=f1, auc=auc, equal=(f1 == f1m and auc == aucm))
    res["ratio"] = res["pooled_ms"] / res["matrix_ms"]
    res["pooled_peak_mb"] = peak_mb(lambda: metrics.pr_roc_pooled(eng, pooled, pooled, pose_xz=xz))
    res["matrix_peak_mb"] = peak_mb(lambda: matrix_path(eng, pooled, xz))
    res["ws_counts_mb"] = eng.score_threshold_counts_workspace_bytes(m, m, eng.MAX_POOLED_THRESHOLDS) / 2**20
    if calls:
        pos, _ = eng.score_positives(pooled, pooled, pose_xz=xz)
        u, mult = metrics.distinct_counts(pos.cpu().numpy())
        above = np.concatenate((np.cumsum(mult[::-1])[::-1], [0])).astype(np.int64)
        step = max(1, -(-u.size // eng.MAX_POOLED_THRESHOLDS))
        thr, rank = u[::step], (u, step, above)
        res["positives"] = int(pos.numel())
        res["positives_ms"], _ = timed(lambda: eng.score_positives(pooled, pooled, pose_xz=xz), reps)
        res["counts_rank_ms"], _ = timed(lambda: eng.score_threshold_counts(pooled, pooled, thr, pose_xz=xz, rank=rank),
                                         reps)
        res["counts_ms"], _ = timed(lambda: eng.score_threshold_counts(pooled, pooled, thr, pose_xz=xz), reps)
        score = eng.score_all_pairs(pooled, pooled)
        res["all_pairs_ms"], _ = timed(lambda: eng.score_all_pairs(pooled, pooled, out=score), reps)
        res["matrix_counts_rank_ms"], _ = timed(lambda: eng.pair_threshold_counts(score, thr, pose_xz=xz, rank=rank), reps)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["kitti", "100k"])
    a = ap.parse_args()
    from oracle import sgpr_oracle
    from sg_pr_amd import allpairs, engine, synth
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.kitti_like_sequence(4541, 100, seed=3)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    xz = allpairs.pose_xz(poses).cuda()
    if a.only in (None, "kitti"):
        case(eng, "kitti00", pooled, xz, a.reps, calls=True)
    if a.only in (None, "100k"):
        reps = -(-100000 // pooled.shape[0])
        big = pooled.repeat(reps, 1)[:100000].contiguous()
        off = torch.arange(reps, device=xz.device, dtype=torch.float64).repeat_interleave(xz.shape[0]) * 1000.0
        bxz = xz.repeat(reps, 1).clone()
        bxz[:, 0] += off
        case(eng, "100k", big, bxz[:100000].contiguous(), max(1, a.reps // 3))
    eng.close()


if __name__ == "__main__":
    main()
