#!/usr/bin/env python3
"""Loop-closure retrieval timings: sgpr_score_topk (fused score + top-k, no matrix) against score_all_pairs + topk_rows.

    python tools/run_topk.py [--reps 10] [--skip-100k]

One JSON line per case: KITTI-00 (4541 x 4541, the synthetic KITTI-like sequence, shipped checkpoint) at k = 1 / 16,
symmetric window 50 and causal; a 100 000-graph database (KITTI-like pooled vectors, each repeated with a small
perturbation) at k = 1 / 16; one query against that database (the online-SLAM latency).  Per case: the median wall
time of each path (CUDA events around the calls, inputs resident), the peak device memory each path adds, and whether
the fused values / indices are bit-equal to the matrix path's (causal cases: the matrix path is the symmetric
score_all_pairs + topk_rows, the same work without the causal rule; no equality).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps):
    for _ in range(2):
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
    out = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20, out


def case(eng, name, rows, cols, k, window, causal, reps, row0=0):
    fused = lambda: eng.score_topk(rows, cols, k=k, window=window, row0=row0, causal=causal)   # noqa: E731
    kk = 1 if k == 1 else 4 if k <= 4 else 8 if k <= 8 else 16

    def matrix():
        score = eng.score_all_pairs(rows, cols)
        return eng.topk_rows(score, k=kk, row0=row0, window=window)

    res = {"case": name, "R": rows.shape[0], "M": cols.shape[0], "k": k, "window": window, "causal": causal}
    res["fused_ms"], f = timed(fused, reps)
    res["fused_peak_mb"], _ = peak_mb(fused)
    try:
        res["matrix_ms"], m = timed(matrix, max(3, reps // 3))
        res["matrix_peak_mb"], _ = peak_mb(matrix)
        if not causal:
            res["bit_equal"] = bool(torch.equal(f[0], m[0][:, :k]) and torch.equal(f[1], m[1][:, :k]))
    except torch.cuda.OutOfMemoryError:
        res["matrix_ms"] = res["matrix_peak_mb"] = None
    torch.cuda.empty_cache()
    res["ws_mb"] = eng.score_topk_workspace_bytes(rows.shape[0], cols.shape[0], k, causal) / 2**20
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-100k", action="store_true")
    opt = ap.parse_args()
    from oracle import sgpr_oracle
    from sg_pr_amd import engine, synth
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, _ = synth.kitti_like_sequence(4541, 100, seed=0)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    for k in (1, 16):
        case(eng, "kitti00_sym_w50", pooled, pooled, k, 50, False, opt.reps)
        case(eng, "kitti00_causal_w50", pooled, pooled, k, 50, True, opt.reps)
    if opt.skip_100k:
        return
    g = torch.Generator(device=pooled.device).manual_seed(1)
    n = 100000
    pick = torch.randint(0, pooled.shape[0], (n,), device=pooled.device, generator=g)
    db = (pooled[pick] + 0.05 * torch.randn(n, pooled.shape[1], device=pooled.device, generator=g)).contiguous()
    for k in (1, 16):
        case(eng, "db100k", db, db, k, 50, False, max(3, opt.reps // 3))
    q = db[n - 1:].contiguous()
    for k in (1, 16):
        case(eng, "db100k_one_query", q, db[:n - 1].contiguous(), k, 50, True, opt.reps, row0=n - 1)


if __name__ == "__main__":
    main()
