"""What a path set buys on a revisit driven at another speed, and what it costs: sgpr_score_path_topk beside
sgpr_score_seq_topk, the path filter beside a device-to-device copy.

    python tools/path_bench.py [--reps N] [--warmup W] [--out profiles/path_bench.txt] [--tiny]

One process, inputs resident.  synth.world_sequence(4541, 100): the last third re-drives the first third.
  recall      the first third is the map.  "slope 2": every 2nd frame of the last third queries it (row i revisits column
              2 i); "slope 1/2": the full last third queries the map thinned to every 2nd frame (row i revisits column
              i // 2).  recall@1 (the listed column lies within 3 m of the query) of single scans (score_topk_large),
              the unit diagonal (score_seq_topk) and the path set {1, 1/2, 2/3, 3/2, 2} (score_path_topk), L in {8, 16},
              both directions, no window (map and query are different frames).  One JSON line each.
  time        the whole sequence against itself, window 50, k in {1, 16}, L in {8, 16}: path_ms / seq_ms (median wall
              time of one call, events around the call, after W warm-up calls), their ratio path_over_seq, and the peak
              device memory of both calls (path_peak_mb, seq_peak_mb).
  filter      the filter alone on one resident score block [4541, 4541] against a copy of that block: filter_ms (9 paths
              and the unit path through seq_path_filter, and seq_filter), copy_ms, filter_over_copy.
--tiny: 240 scans, 2 repetitions (a smoke run; writes no file unless --out is given).  Per-kernel times: run the same
command under `rocprofv3 --kernel-trace --stats -- python tools/path_bench.py`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SLOPES = ("1", "1/2", "2/3", "3/2", "2")
LENGTHS, KS = (8, 16), (1, 16)


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


def recall_at_1(idx, query_xz, map_xz, p_thresh=3.0):
    """share of the queries whose listed column lies within p_thresh of them (a padding slot counts as a miss)"""
    col = idx[:, 0].cpu().numpy()
    ok = col >= 0
    d = np.linalg.norm(query_xz - map_xz[np.maximum(col, 0)], axis=1)
    return float(np.mean(ok & (d <= p_thresh)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=4541)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if opt.tiny:
        opt.graphs, opt.reps, opt.warmup = 240, 2, 1
    elif opt.out is None:
        opt.out = os.path.join(REPO, "profiles", "path_bench.txt")
    from sg_pr_amd import engine, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.world_sequence(opt.graphs, 100)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    xz = np.asarray(poses, dtype=np.float64)[:, [3, 11]]
    n, third = opt.graphs, opt.graphs // 3
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    cases = (("slope 2", np.arange(n - third, n, 2), np.arange(third)),
             ("slope 1/2", np.arange(n - third, n), np.arange(0, third, 2)))
    for name, q_ids, m_ids in cases:
        rows = pooled[torch.from_numpy(q_ids).cuda()].contiguous()
        cols = pooled[torch.from_numpy(m_ids).cuda()].contiguous()
        single = recall_at_1(eng.score_topk_large(rows, cols, k=1)[1], xz[q_ids], xz[m_ids])
        for L in LENGTHS:
            paths = engine.seq_paths(L, SLOPES)
            unit = recall_at_1(eng.score_seq_topk(rows, cols, L, k=1)[1], xz[q_ids], xz[m_ids])
            v, i, c = eng.score_path_topk(rows, cols, L, paths, k=1)
            code = c[:, 0].cpu().numpy()
            listed = (i[:, 0] >= 0).cpu().numpy()
            share = np.bincount(code[listed] >> 1, minlength=paths.shape[0]) / max(int(listed.sum()), 1)
            emit({"case": name, "queries": len(q_ids), "map": len(m_ids), "seq_len": L, "paths": int(paths.shape[0]),
                  "recall1_single": round(single, 4), "recall1_unit": round(unit, 4),
                  "recall1_paths": round(recall_at_1(i, xz[q_ids], xz[m_ids]), 4),
                  "share_per_path": [round(float(x), 3) for x in share]})
    for L in LENGTHS:
        paths = engine.seq_paths(L, SLOPES)
        for k in KS:
            def seq():
                return eng.score_seq_topk(pooled, pooled, L, k=k, window=50)

            def path():
                return eng.score_path_topk(pooled, pooled, L, paths, k=k, window=50)
            seq_ms, path_ms = median_ms(seq, opt.reps, opt.warmup), median_ms(path, opt.reps, opt.warmup)
            emit({"shape": "square", "rows": n, "cols": n, "seq_len": L, "k": k, "paths": int(paths.shape[0]),
                  "path_ms": round(path_ms, 3), "seq_ms": round(seq_ms, 3), "path_over_seq": round(path_ms / seq_ms, 3),
                  "path_peak_mb": round(peak_mb(path), 1), "seq_peak_mb": round(peak_mb(seq), 1)})
    block = eng.score_all_pairs(pooled, pooled)
    dst = torch.empty_like(block)
    code = torch.empty(block.shape, dtype=torch.uint8, device=block.device)
    copy_ms = median_ms(lambda: dst.copy_(block), opt.reps, opt.warmup)
    for L in LENGTHS:
        paths = engine.seq_paths(L, SLOPES)
        runs = (("paths", lambda: eng.seq_path_filter(block, L, paths, reverse="both", out=dst, out_code=code)),
                ("unit path", lambda: eng.seq_path_filter(block, L, engine.seq_paths(L, ["1"]), reverse="both", out=dst,
                                                          out_code=code)),
                ("seq_filter", lambda: eng.seq_filter(block, L, reverse="both", out=dst, out_dir=code)))
        for what, fn in runs:
            ms = median_ms(fn, opt.reps, opt.warmup)
            emit({"filter": what, "rows": n, "cols": n, "seq_len": L, "paths": int(paths.shape[0]) if what == "paths" else 1,
                  "filter_ms": round(ms, 4), "copy_ms": round(copy_ms, 4), "filter_over_copy": round(ms / copy_ms, 2)})
    eng.close()
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("# python tools/path_bench.py --reps %d --warmup %d --graphs %d (MI355X; times in ms, medians)\n"
                    % (opt.reps, opt.warmup, opt.graphs))
            f.write("\n".join(json.dumps(r) for r in records) + "\n")
    return records


if __name__ == "__main__":
    main()
