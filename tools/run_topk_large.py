#!/usr/bin/env python3
"""Large-k loop-closure timings (sgpr_topk_rows_large, sgpr_score_topk_large).

    python tools/run_topk_large.py [--reps 10] [--skip-100k] [--out profiles/r10_topk_large.txt]

One JSON line per case, also written to --out: the resident KITTI-00 matrix (4541 x 4541, synthetic KITTI-like
sequence, shipped checkpoint) at k = 45 (window 50) and k = 1000 beside sgpr_topk_rows at k = 16; the pooled KITTI-00
rectangle at k = 45, window 50, symmetric and causal, beside score_all_pairs + torch.topk on the masked matrix and
sgpr_score_topk at k = 16; one query against a 100 000-frame database at k = 1000 (causal) and the 100 000 x 100 000
map at k = 1000 (recall@1 %), beside sgpr_score_topk at k = 16.  Per case: the median wall time (CUDA events, inputs
resident), the peak device memory the call adds, and whether the values / indices are torch.equal to the masked stable
sort of the same handle's score_all_pairs matrix (at 100 k on the first, a middle and the last 64 MB row block).
Kernel times and the selection's share: run it under `rocprofv3 --kernel-trace --stats` (a run of its own) and keep the
stats as profiles/r10_topk_large_kernels.txt.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from run_topk import peak_mb, timed  # noqa: E402


def masked_sort(score, k, window=-1, row0=0, causal=False):
    """the reference: ineligible columns and NaN to -inf, stable descending sort, (-inf, -1) where nothing qualifies"""
    r, m = score.shape
    s = score.clone()
    s[torch.isnan(s)] = -float("inf")
    self_ = torch.arange(r, device=s.device) + row0
    c = torch.arange(m, device=s.device)
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


def torch_route(eng, rows, cols, k, window, causal, row0=0):
    """score_all_pairs + torch.topk on the masked matrix (the route users have without the large-k entry points)"""
    score = eng.score_all_pairs(rows, cols)
    r, m = score.shape
    self_ = torch.arange(r, device=score.device) + row0
    c = torch.arange(m, device=score.device)
    bad = (c[None, :] - self_[:, None]).abs() <= window
    if causal:
        bad |= c[None, :] >= self_[:, None]
    score.masked_fill_(bad, -float("inf"))
    return torch.topk(score, k, dim=1)


def emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-100k", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10_topk_large.txt"))
    opt = ap.parse_args()
    from oracle import sgpr_oracle
    from sg_pr_amd import engine, synth
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, _ = synth.kitti_like_sequence(4541, 100, seed=0)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    out = open(opt.out, "w")

    # resident KITTI-00 matrix
    score = eng.score_all_pairs(pooled, pooled)
    base_ms, _ = timed(lambda: eng.topk_rows(score, k=16, window=50), opt.reps)
    for k, target in ((45, 0.060), (1000, 0.120)):
        fn = lambda: eng.topk_rows_large(score, k=k, window=50)   # noqa: E731
        ms, got = timed(fn, opt.reps)
        peak, _ = peak_mb(fn)
        ok = all(torch.equal(a, b) for a, b in zip(got, masked_sort(score, k, window=50)))
        emit({"case": "resident_kitti00_w50", "R": 4541, "M": 4541, "k": k, "ms": ms, "peak_mb": peak,
              "topk_rows_k16_ms": base_ms, "target_ms": target, "met": ms <= target, "equal": ok}, out)
    del score

    # pooled KITTI-00 rectangle
    for causal in (False, True):
        k16_ms, _ = timed(lambda: eng.score_topk(pooled, pooled, k=16, window=50, causal=causal), opt.reps)
        tr_ms, _ = timed(lambda: torch_route(eng, pooled, pooled, 45, 50, causal), opt.reps)
        fn = lambda: eng.score_topk_large(pooled, pooled, k=45, window=50, causal=causal)   # noqa: E731
        ms, got = timed(fn, opt.reps)
        peak, _ = peak_mb(fn)
        ok = all(torch.equal(a, b) for a, b in zip(got, masked_sort(eng.score_all_pairs(pooled, pooled), 45, 50,
                                                                    causal=causal)))
        emit({"case": "pooled_kitti00_w50", "causal": causal, "R": 4541, "M": 4541, "k": 45, "ms": ms, "peak_mb": peak,
              "torch_route_ms": tr_ms, "score_topk_k16_ms": k16_ms, "target_ms": 0.25,
              "met": ms <= 0.25 and ms < tr_ms, "equal": ok}, out)
    if opt.skip_100k:
        return
    g = torch.Generator(device=pooled.device).manual_seed(1)
    n = 100000
    pick = torch.randint(0, pooled.shape[0], (n,), device=pooled.device, generator=g)
    db = (pooled[pick] + 0.05 * torch.randn(n, pooled.shape[1], device=pooled.device, generator=g)).contiguous()

    # one query against 100 000 frames
    q, cols = db[n - 1:].contiguous(), db[:n - 1].contiguous()
    k16_ms, _ = timed(lambda: eng.score_topk(q, cols, k=16, window=50, row0=n - 1, causal=True), opt.reps)
    fn = lambda: eng.score_topk_large(q, cols, k=1000, window=50, row0=n - 1, causal=True)   # noqa: E731
    ms, got = timed(fn, opt.reps)
    peak, _ = peak_mb(fn)
    ok = all(torch.equal(a, b) for a, b in zip(got, masked_sort(eng.score_all_pairs(q, cols), 1000, 50, n - 1, True)))
    emit({"case": "one_query_100k_causal", "R": 1, "M": n - 1, "k": 1000, "ms": ms, "peak_mb": peak,
          "score_topk_k16_ms": k16_ms, "target_ms": 0.30, "met": ms <= 0.30, "equal": ok}, out)

    # the 100 000 x 100 000 map, recall@1 % (k = 1000)
    reps = max(3, opt.reps // 3)
    k16_ms, _ = timed(lambda: eng.score_topk(db, db, k=16, window=50), reps)
    fn = lambda: eng.score_topk_large(db, db, k=1000, window=50)   # noqa: E731
    ms, got = timed(fn, reps)
    peak, _ = peak_mb(fn)
    rb = max(1, min(n, (64 << 20) // (4 * n)))
    ok = True
    for b0 in (0, rb * ((n // rb) // 2), rb * ((n - 1) // rb)):
        rows = db[b0:b0 + rb].contiguous()
        want = masked_sort(eng.score_all_pairs(rows, db), 1000, 50, row0=b0)
        ok = ok and all(torch.equal(a[b0:b0 + rb], b) for a, b in zip(got, want))
    out_mb = n * 1000 * 8 / 2**20
    emit({"case": "map_100k_recall1pct", "R": n, "M": n, "k": 1000, "ms": ms, "peak_mb": peak, "output_mb": out_mb,
          "score_topk_k16_ms": k16_ms, "target_ms": 1.3 * k16_ms, "met": ms <= 1.3 * k16_ms and peak - out_mb <= 1024,
          "equal_sampled_blocks": ok}, out)
    out.close()


if __name__ == "__main__":
    main()
