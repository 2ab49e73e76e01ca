"""Time sgpr_score_mine against sgpr_score_topk and the matrix path on a KITTI-00-sized sequence (4541 x 4541).

    python tools/mine_bench.py [--reps N] [--warmup W]

Inputs are resident; every figure is the median wall time of one call (CUDA events around the call, after W warm-up
calls).  The matrix path is score_all_pairs + mine_rows on the resident matrix.  Per-kernel times: run the same
command under `rocprofv3 --kernel-trace --stats -- python tools/mine_bench.py`."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=4541)
    opt = ap.parse_args()
    from sg_pr_amd import engine, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.world_sequence(opt.graphs, 100, seed=7)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    xz = torch.from_numpy(np.ascontiguousarray(poses[:, [3, 11]])).cuda()
    score = eng.score_all_pairs(pooled, pooled)
    torch.cuda.synchronize()
    rows = []
    for k in (1, 16):
        rec = {"graphs": opt.graphs, "k": k, "window": 50}
        rec["topk_ms"] = median_ms(lambda: eng.score_topk(pooled, pooled, k=k, window=50), opt.reps, opt.warmup)
        for name, pos in (("neg", False), ("pos", True)):
            rec["mine_%s_ms" % name] = median_ms(
                lambda: eng.score_mine(pooled, pooled, xz, k=k, positives=pos, window=50), opt.reps, opt.warmup)
            rec["matrix_%s_ms" % name] = median_ms(
                lambda: eng.mine_rows(eng.score_all_pairs(pooled, pooled, out=score), xz, k=k, positives=pos, window=50),
                opt.reps, opt.warmup)
            rec["mine_%s_over_topk" % name] = round(rec["mine_%s_ms" % name] / rec["topk_ms"], 3)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
