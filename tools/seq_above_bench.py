"""Time sgpr_score_seq_above against the three calls it replaces, and pr_roc_seq_pooled against the filtered matrix.

    python tools/seq_above_bench.py [--reps N] [--warmup W] [--out profiles/seq_above.txt]

Two shapes, in one process: a KITTI-00-sized sequence against itself (4541 x 4541, synth.world_sequence) and one query
with its L - 1 context rows against a 100 000-frame map (random pooled vectors).  For L in {1, 8, 32}, forward and both
directions, window 50 and a threshold that about 0.1 % of the entries of Q reach (read off the filtered matrix), one
JSON line each with the median wall time (events around the calls, after W warm-up runs) and the peak device memory
(workspaces and outputs) of three routes, every capacity sized to the count so that no route reads anything back:
  fused_*    (a) score_seq_above
  matrix_*   (b) score_all_pairs + seq_filter with dir + rows_above on the same rows (the directions stay in the dir
             matrix: gathering them would be a fourth call)
  plain_*    (c) score_above on the single-scan score at a threshold that takes as many pairs: the floor
and, at the square shape, pr_roc_seq_pooled beside score_all_pairs + seq_filter + pr_roc_device (eval_*).  Route (a) is
checked against route (b) bit for bit before anything is timed.  Inputs are resident.
Per-kernel times: run the same command under `rocprofv3 --kernel-trace --stats -- python tools/seq_above_bench.py`."""
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


def value_at(t, keep):
    """the value that a fraction `keep` of the entries of t reach"""
    flat = t.flatten()
    return float(flat.kthvalue(max(1, flat.numel() - int(flat.numel() * keep)))[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=4541)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--keep", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seq_above.txt"))
    opt = ap.parse_args()
    from sg_pr_amd import allpairs, engine, metrics, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.world_sequence(opt.graphs, 100, seed=7)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    xz = allpairs.pose_xz(poses).cuda()
    g = torch.Generator().manual_seed(1)
    big = (torch.randn(opt.map, eng.pw, generator=g) * 3.0).cuda()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for L in (1, 8, 32):
        shapes = (("square", pooled, pooled, 0), ("one query", big[:L].contiguous(), big, L - 1))
        for name, rows, cols, ctx in shapes:
            for dname, reverse in (("forward", False), ("both", "both")):
                score = eng.score_all_pairs(rows, cols)
                thr = value_at(eng.seq_filter(score, L, context=ctx, reverse=reverse), opt.keep)
                thr_plain = value_at(score[ctx:], opt.keep)
                del score
                kw = dict(window=50, context=ctx, reverse=reverse)
                want = eng.score_seq_above(rows, cols, L, thr, **kw)
                n = want[0].numel()
                n_plain = eng.score_above(rows[ctx:].contiguous(), cols, thr_plain, window=50, row0=ctx)[0].numel()

                def fused():
                    return eng.score_seq_above(rows, cols, L, thr, capacity=n, **kw)

                def matrix():
                    q, d = eng.seq_filter(eng.score_all_pairs(rows, cols), L, context=ctx, reverse=reverse, want_dir=True)
                    return eng.rows_above(q, thr, window=50, row0=ctx, capacity=n) + (d,)

                plain_rows = rows[ctx:].contiguous()

                def plain():
                    return eng.score_above(plain_rows, cols, thr_plain, window=50, row0=ctx, capacity=n_plain)

                got, ref = fused(), matrix()
                same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                       b.view(torch.int32) if b.dtype == torch.float32 else b)
                           for a, b in zip(got[:3] + (got[4],), ref[:4]))
                same = same and torch.equal(got[3], ref[4][got[0].long(), got[1].long()])
                rec = {"shape": name, "rows": rows.shape[0], "cols": cols.shape[0], "context": ctx, "seq_len": L,
                       "directions": dname, "threshold": thr, "pairs": n, "plain_pairs": n_plain, "equal": bool(same)}
                del got, ref, want
                for key, fn in (("fused", fused), ("matrix", matrix), ("plain", plain)):
                    rec[key + "_ms"] = round(median_ms(fn, opt.reps, opt.warmup), 3)
                    rec[key + "_peak_mb"] = peak_mb(fn)
                rec["fused_over_matrix"] = round(rec["fused_ms"] / rec["matrix_ms"], 3)
                rec["fused_over_plain"] = round(rec["fused_ms"] / rec["plain_ms"], 3)
                emit(rec)
        for dname, reverse in (("forward", False), ("both", "both")):
            def eval_pooled():
                return metrics.pr_roc_seq_pooled(eng, pooled, pooled, L, pose_xz=xz, reverse=reverse)

            def eval_matrix():
                q = eng.seq_filter(eng.score_all_pairs(pooled, pooled), L, reverse=reverse)
                return metrics.pr_roc_device(eng, q, pose_xz=xz)
            a, b = eval_pooled(), eval_matrix()
            rec = {"shape": "square", "frames": pooled.shape[0], "seq_len": L, "directions": dname, "f1_max": a[0],
                   "roc_auc": a[1], "equal": bool(a[:2] == b[:2]), "passes_pooled": a[2], "passes_matrix": b[2]}
            reps = max(3, opt.reps // 4)
            for key, fn in (("eval_pooled", eval_pooled), ("eval_matrix", eval_matrix)):
                rec[key + "_ms"] = round(median_ms(fn, reps, 1), 3)
                rec[key + "_peak_mb"] = peak_mb(fn)
            emit(rec)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("# python tools/seq_above_bench.py --reps %d --warmup %d --keep %g (MI355X; times in ms, medians)\n"
                % (opt.reps, opt.warmup, opt.keep))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
