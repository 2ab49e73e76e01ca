#!/usr/bin/env python3
"""Range retrieval timings: sgpr_score_above (fused two-pass score + selection, no matrix) against score_all_pairs +
rows_above (row-blocked beyond 64 M entries).

    python tools/run_above.py [--reps 10] [--only kitti|100k]
    python tools/run_above.py --summarise <rocprofv3 kernel_trace.csv>

One JSON line per case: KITTI-00 (4541 x 4541, the synthetic KITTI-like sequence, shipped checkpoint) and a 100 000-graph
database (KITTI-like pooled vectors, each repeated with a small perturbation), at thresholds that keep about 1e-3 and
1e-5 of the pairs, window 50, symmetric and causal.  Per case: the median wall time of each path (CUDA events around the
calls, inputs resident, capacity sized to the count so that each is one asynchronous call), the peak device memory each
path adds, the pair count and whether both paths return the same bytes; the 100 k cases also time score_topk at k = 1.
Kernel times: run it under `rocprofv3 --kernel-trace --stats` and pass the trace to --summarise (medians per kernel;
score_above_kernel's dispatches are split into pass 1 - the one followed by above_fold_kernel - and pass 2).
"""
import argparse
import csv
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


def matrix_path(eng, rows, cols, thr, window, causal, cap):
    """score_all_pairs + rows_above, in row blocks of at most 64 M entries (the whole matrix when it fits)"""
    r, m = rows.shape[0], cols.shape[0]
    rb = max(1, min(r, (64 << 20) // m))
    if rb == r:
        return eng.rows_above(eng.score_all_pairs(rows, cols), thr, window=window, causal=causal, capacity=cap)
    buf = torch.empty(rb, m, dtype=torch.float32, device=rows.device)
    parts, counts = [], []
    for r0 in range(0, r, rb):
        n = min(rb, r - r0)
        eng.score_all_pairs(rows[r0:r0 + n], cols, out=buf[:n])
        out = eng.rows_above(buf[:n], thr, window=window, row0=r0, causal=causal)
        parts.append((out[0] + r0, out[1], out[2]))
        counts.append(out[3][1:] - out[3][:-1])
    rp = torch.zeros(r + 1, dtype=torch.int64, device=rows.device)
    rp[1:] = torch.cumsum(torch.cat(counts), 0)
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3)) + (rp,)


def case(eng, name, rows, cols, thr, keep, window, causal, reps, topk=False):
    r, m = rows.shape[0], cols.shape[0]
    count = int(eng.score_above(rows, cols, thr, window=window, causal=causal, capacity=0)[3][-1])
    fused = lambda: eng.score_above(rows, cols, thr, window=window, causal=causal, capacity=count)   # noqa: E731
    res = {"case": name, "R": r, "M": m, "keep": keep, "threshold": thr, "window": window, "causal": causal,
           "pairs": count}
    res["fused_ms"], f = timed(fused, reps)
    res["fused_peak_mb"], _ = peak_mb(fused)
    mreps = max(3, reps // 3)
    res["matrix_ms"], mat = timed(lambda: matrix_path(eng, rows, cols, thr, window, causal, count), mreps)
    res["matrix_peak_mb"], _ = peak_mb(lambda: matrix_path(eng, rows, cols, thr, window, causal, count))
    res["bit_equal"] = all(torch.equal(a, b) for a, b in zip(f, mat))
    if topk:
        res["topk1_ms"], _ = timed(lambda: eng.score_topk(rows, cols, k=1, window=window, causal=causal), mreps)
    res["ws_mb"] = eng.score_above_workspace_bytes(r, m, causal) / 2**20
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    return res


def thresholds(score, keeps):
    v = score.flatten().sort(descending=True).values
    return [float(v[max(0, int(k * v.numel()) - 1)]) for k in keeps]


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    groups = {}
    for i, x in enumerate(rows):
        name = x["Kernel_Name"].split("(")[0].replace("sgpr::", "").replace("void ", "")
        if name.startswith("score_above_kernel"):
            nxt = rows[i + 1]["Kernel_Name"] if i + 1 < len(rows) else ""
            name += " pass 1" if "above_fold_kernel" in nxt else " pass 2"
        groups.setdefault(name, []).append((int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1000.0)
    for name, ts in sorted(groups.items()):
        ts.sort()
        print("  %-52s n=%4d  median %10.1f us  min %10.1f us" % (name[:52], len(ts), ts[len(ts) // 2], ts[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["kitti", "100k"])
    ap.add_argument("--summarise")
    opt = ap.parse_args()
    if opt.summarise:
        summarise(opt.summarise)
        return
    from oracle import sgpr_oracle
    from sg_pr_amd import engine, synth
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, _ = synth.kitti_like_sequence(4541, 100, seed=0)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    keeps = (1e-3, 1e-5)
    if opt.only != "100k":
        thr = thresholds(eng.score_all_pairs(pooled, pooled), keeps)
        for t, keep in zip(thr, keeps):
            for causal in (False, True):
                case(eng, "kitti00_w50", pooled, pooled, t, keep, 50, causal, opt.reps)
    if opt.only == "kitti":
        return
    g = torch.Generator(device=pooled.device).manual_seed(1)
    n = 100000
    pick = torch.randint(0, pooled.shape[0], (n,), device=pooled.device, generator=g)
    db = (pooled[pick] + 0.05 * torch.randn(n, pooled.shape[1], device=pooled.device, generator=g)).contiguous()
    thr = thresholds(eng.score_all_pairs(db[:2000], db), keeps)      # from a 2000-row sample of the matrix
    torch.cuda.empty_cache()
    for t, keep in zip(thr, keeps):
        for causal in (False, True):
            case(eng, "db100k_w50", db, db, t, keep, 50, causal, max(3, opt.reps // 3), topk=True)


if __name__ == "__main__":
    main()
