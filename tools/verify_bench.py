"""Time the geometric verification (sgpr_verify_pairs) of top-k loop-closure lists on a synthetic world sequence.

    python tools/verify_bench.py [--graphs G] [--node-num N] [--k K] [--reps N] [--warmup W] [--out FILE]

The graphs are resident on the device; every time is the median wall time of one call (events around the call, after W
warm-up calls) - the verification is ONE kernel, so its wall time is the kernel time plus one launch.  Beside it: the
retrieval call that produced the lists (score_topk on the pooled vectors), the distribution of the `hypotheses` field,
the inliers of true and false candidates and recall@1 before and after re-ranking.  Prints one JSON line."""
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4541)
    ap.add_argument("--node-num", type=int, default=100)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--min-inliers", type=int, default=12)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args(argv)
    from sg_pr_amd import engine, metrics, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.world_sequence(opt.graphs, opt.node_num, seed=0)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
    vals, idx = eng.score_topk(pooled, pooled, k=opt.k, window=opt.window)
    m, k = idx.shape
    rows = torch.arange(m, dtype=torch.int32, device=idx.device).repeat_interleave(k)
    cols = idx.reshape(-1).contiguous()
    torch.cuda.synchronize()
    res = engine.verify_pairs(dc, dl, dc, dl, rows, cols)
    torch.cuda.synchronize()
    rec = {"graphs": m, "node_num": opt.node_num, "k": k, "window": opt.window, "pairs": int(rows.numel())}
    rec["retrieval_ms"] = median_ms(lambda: eng.score_topk(pooled, pooled, k=opt.k, window=opt.window), opt.reps, opt.warmup)
    rec["verify_ms"] = median_ms(lambda: engine.verify_pairs(dc, dl, dc, dl, rows, cols), opt.reps, opt.warmup)
    rec["us_per_pair"] = 1e3 * rec["verify_ms"] / max(rec["pairs"], 1)
    rec["pairs_per_s"] = rec["pairs"] / (1e-3 * rec["verify_ms"]) if rec["verify_ms"] > 0 else 0.0
    rec["verify_over_retrieval"] = rec["verify_ms"] / rec["retrieval_ms"] if rec["retrieval_ms"] > 0 else 0.0
    valid = (cols >= 0).cpu().numpy()
    hyp = res["hypotheses"].cpu().numpy()[valid]
    inl = res["inliers_refined"].cpu().numpy()[valid]
    flags = res["flags"].cpu().numpy()[valid]
    xz = poses[:, [3, 11]]
    r, c = rows.cpu().numpy()[valid], cols.cpu().numpy()[valid]
    dist = np.hypot(*(xz[r] - xz[c]).T)
    true, false = dist <= 3.0, dist >= 20.0
    rec["hypotheses_median"] = float(np.median(hyp)) if hyp.size else 0.0
    rec["hypotheses_max"] = int(hyp.max()) if hyp.size else 0
    rec["truncated"] = int(((flags & engine.VERIFY_TRUNCATED) != 0).sum())
    rec["no_hypothesis"] = int(((flags & engine.VERIFY_NO_HYPOTHESIS) != 0).sum())
    rec["true_candidates"] = int(true.sum())
    rec["false_candidates"] = int(false.sum())
    rec["true_inliers_median"] = float(np.median(inl[true])) if true.any() else 0.0
    rec["true_inliers_min"] = int(inl[true].min()) if true.any() else 0
    rec["false_inliers_max"] = int(inl[false].max()) if false.any() else 0
    acc = inl >= opt.min_inliers
    rec["accepted"] = int(acc.sum())
    rec["accepted_precision"] = float(true[acc].sum() / max((true | false)[acc].sum(), 1))
    err = metrics.closure_pose_errors({"refined": res["refined"].cpu().numpy()[valid][acc & true], "flags": flags[acc & true]},
                                      r[acc & true], c[acc & true], poses)
    rec["median_yaw_deg"] = err["median_yaw_deg"] if (acc & true).any() else 0.0
    rec["median_trans_m"] = err["median_trans_m"] if (acc & true).any() else 0.0
    # recall@1 of the lists as retrieved and re-ranked by (refined inliers, score, column)
    inl2 = torch.where(idx >= 0, res["inliers_refined"].reshape(m, k), torch.full_like(idx, -1))
    o = torch.argsort(torch.where(idx >= 0, idx, torch.full_like(idx, 0x7fffffff)), dim=1, stable=True)
    o = o.gather(1, torch.argsort(-vals.gather(1, o), dim=1, stable=True))
    o = o.gather(1, torch.argsort(-inl2.gather(1, o), dim=1, stable=True))
    rec["recall1"] = float(metrics.recall_at_n(idx, poses, window=opt.window)[0])
    rec["recall1_reranked"] = float(metrics.recall_at_n(idx.gather(1, o), poses, window=opt.window)[0])
    line = json.dumps(rec)
    print(line, flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    return rec


if __name__ == "__main__":
    main()
