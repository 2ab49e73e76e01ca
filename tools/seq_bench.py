"""Time sgpr_score_seq_topk against sgpr_score_topk_large, and the diagonal filter against a device-to-device copy.

    python tools/seq_bench.py [--reps N] [--warmup W] [--out profiles/r09_seq.txt]

Two shapes, in one process: a KITTI-00-sized sequence against itself (4541 x 4541, synth.world_sequence) and one query
with its L - 1 context rows against a 100 000-frame map (random pooled vectors).  For k in {1, 16}, L in {1, 8, 32},
forward and both directions, one JSON line each with
  seq_ms / topk_large_ms   median wall time of one call (events around the call, after W warm-up calls); the baseline is
                           score_topk_large on the same rows, columns and k - at L = 1 the new call does the same work
                           plus the filter
  seq_peak_mb / topk_large_peak_mb   peak device memory allocated during one call (the workspace and the outputs)
then, per shape and L, the filter alone on one resident score block against a copy of that block (filter_ms, copy_ms,
filter_over_copy), and recall@1 of the world sequence at L = 1 and L = 8 (window 50, 3 m).  Inputs are resident.
Per-kernel times: run the same command under `rocprofv3 --kernel-trace --stats -- python tools/seq_bench.py`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


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
    return round((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=4541)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09_seq.txt"))
    opt = ap.parse_args()
    from sg_pr_amd import engine, metrics, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.world_sequence(opt.graphs, 100, seed=7)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    g = torch.Generator().manual_seed(1)
    big = (torch.randn(opt.map, eng.pw, generator=g) * 3.0).cuda()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for L in (1, 8, 32):
        shapes = (("square", pooled, pooled, 0), ("one query", big[:L].contiguous(), big, L - 1))
        for name, rows, cols, ctx in shapes:
            for k in (1, 16):
                rec = {"shape": name, "rows": rows.shape[0], "cols": cols.shape[0], "context": ctx, "seq_len": L, "k": k}

                def base():
                    return eng.score_topk_large(rows, cols, k=k, window=50)
                rec["topk_large_ms"] = round(median_ms(base, opt.reps, opt.warmup), 3)
                rec["topk_large_peak_mb"] = peak_mb(base)
                for dname, reverse in (("forward", False), ("both", "both")):
                    def seq():
                        return eng.score_seq_topk(rows, cols, L, k=k, window=50, context=ctx, reverse=reverse)
                    rec["seq_%s_ms" % dname] = round(median_ms(seq, opt.reps, opt.warmup), 3)
                    rec["seq_%s_peak_mb" % dname] = peak_mb(seq)
                    rec["seq_%s_over_topk_large" % dname] = round(rec["seq_%s_ms" % dname] / rec["topk_large_ms"], 3)
                emit(rec)
            # the filter alone on one resident block of the call, against a copy of the same block
            rb = max(1, min(rows.shape[0], (64 << 20) // (4 * cols.shape[0])))
            block = eng.score_all_pairs(rows[:rb].contiguous(), cols)
            c = min(ctx, rb - 1)
            q = torch.empty(rb - c, cols.shape[0], dtype=torch.float32, device=block.device)
            d = torch.empty(rb - c, cols.shape[0], dtype=torch.uint8, device=block.device)
            dst = torch.empty_like(block)
            rec = {"shape": name, "block_rows": rb, "cols": cols.shape[0], "context": c, "seq_len": L,
                   "copy_ms": round(median_ms(lambda: dst.copy_(block), opt.reps, opt.warmup), 4)}
            for dname, reverse, od in (("forward", False, None), ("both", "both", d)):
                ms = median_ms(lambda: eng.seq_filter(block, L, context=c, reverse=reverse, out=q, out_dir=od), opt.reps,
                               opt.warmup)
                rec["filter_%s_ms" % dname] = round(ms, 4)
                rec["filter_%s_over_copy" % dname] = round(ms / rec["copy_ms"], 2)
            emit(rec)
    for L in (1, 8):
        idx = eng.score_seq_topk(pooled, pooled, L, k=1, window=50)[1]
        rec1 = metrics.recall_at_n(idx, poses, p_thresh=3.0, window=50)
        emit({"world_sequence": opt.graphs, "seq_len": L, "window": 50, "recall_at_1": round(float(rec1[0]), 4)})
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("# python tools/seq_bench.py --reps %d --warmup %d (MI355X; times in ms, medians)\n" % (opt.reps, opt.warmup))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
