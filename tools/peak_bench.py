"""Time sgpr_score_peak_topk against the plain list calls, and the peak filter against a device-to-device copy.

    python tools/peak_bench.py [--reps N] [--warmup W] [--out profiles/peak_bench.txt] [--tiny]

Two shapes, in one process, inputs resident: synth.world_sequence(4541, 100) against itself and one query (with its
L - 1 context rows) against a 100 000-frame map of random pooled vectors.  For k in {4, 16}, rho in {0, 10, 50, 1024}
and L in {1, 8}, one JSON line each with
  peak_ms / plain_ms      median wall time of one call (events around the call, after W warm-up calls); the plain call is
                          score_topk_large (L = 1) or score_seq_topk (L = 8) on the same rows, columns and k
  peak_over_plain         their ratio - what distinct lists cost at equal k
  added_peak_mb           peak device memory allocated during the distinct call minus that of the plain call
  places_per_list(_plain) mean number of places per list (metrics.places_per_list at rho; rho = 0: at 10) - square shape
then, per shape and rho, the filter alone on one resident score block against a copy of that block (filter_ms, copy_ms,
filter_over_copy).  --tiny: 200 scans, a 3000-frame map, 2 repetitions (a smoke run; writes no file unless --out is
given).  Per-kernel times: run the same command under `rocprofv3 --kernel-trace --stats -- python tools/peak_bench.py`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KS, RADII, LENGTHS = (4, 16), (0, 10, 50, 1024), (1, 8)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=4541)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if opt.tiny:
        opt.graphs, opt.map, opt.reps, opt.warmup = 200, 3000, 2, 1
    elif opt.out is None:
        opt.out = os.path.join(REPO, "profiles", "peak_bench.txt")
    from sg_pr_amd import engine, metrics, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.world_sequence(opt.graphs, 100)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    g = torch.Generator().manual_seed(1)
    big = (torch.randn(opt.map, eng.pw, generator=g) * 3.0).cuda()
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for L in LENGTHS:
        shapes = (("square", pooled, pooled, 0), ("one query", big[:L].contiguous(), big, L - 1))
        for name, rows, cols, ctx in shapes:
            for k in KS:
                if L == 1:
                    def plain():
                        return eng.score_topk_large(rows, cols, k=k, window=50)
                else:
                    def plain():
                        return eng.score_seq_topk(rows, cols, L, k=k, window=50, context=ctx, reverse="both")
                plain_ms, plain_mb = median_ms(plain, opt.reps, opt.warmup), peak_mb(plain)
                plain_idx = plain()[1]
                for rho in RADII:
                    def distinct():
                        return eng.score_peak_topk(rows, cols, rho, seq_len=L, k=k, window=50, context=ctx,
                                                   reverse="both" if L > 1 else False)
                    ms = median_ms(distinct, opt.reps, opt.warmup)
                    rec = {"shape": name, "rows": rows.shape[0], "cols": cols.shape[0], "context": ctx, "seq_len": L,
                           "k": k, "radius": rho, "peak_ms": round(ms, 3), "plain_ms": round(plain_ms, 3),
                           "peak_over_plain": round(ms / plain_ms, 3),
                           "added_peak_mb": round(peak_mb(distinct) - plain_mb, 1)}
                    if name == "square":
                        at = rho if rho > 0 else 10
                        rec["places_per_list"] = round(metrics.places_per_list(distinct()[1], at), 3)
                        rec["places_per_list_plain"] = round(metrics.places_per_list(plain_idx, at), 3)
                    emit(rec)
        # the filter alone on one resident block of each shape, against a copy of the same block
        if L == 1:
            for name, rows, cols, ctx in shapes:
                rb = max(1, min(rows.shape[0], (64 << 20) // (4 * cols.shape[0])))
                block = eng.score_all_pairs(rows[:rb].contiguous(), cols)
                dst = torch.empty_like(block)
                copy_ms = median_ms(lambda: dst.copy_(block), opt.reps, opt.warmup)
                for rho in RADII:
                    ms = median_ms(lambda: eng.peak_filter(block, rho, window=50, out=dst), opt.reps, opt.warmup)
                    emit({"shape": name, "block_rows": rb, "cols": cols.shape[0], "radius": rho,
                          "filter_ms": round(ms, 4), "copy_ms": round(copy_ms, 4),
                          "filter_over_copy": round(ms / copy_ms, 2)})
    eng.close()
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("# python tools/peak_bench.py --reps %d --warmup %d --graphs %d --map %d (MI355X; times in ms, medians)\n"
                    % (opt.reps, opt.warmup, opt.graphs, opt.map))
            f.write("\n".join(json.dumps(r) for r in records) + "\n")
    return records


if __name__ == "__main__":
    main()
