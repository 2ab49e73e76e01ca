"""Time sgpr_score_session_above against the three calls it replaces and against sgpr_score_seq_above.

    python tools/session_above_bench.py [--reps N] [--warmup W] [--small] [--out profiles/session_above_bench.txt]

Two shapes, in one process: a KITTI-00-sized sequence against itself (4541 x 4541, synth.world_sequence) and one query
with its L - 1 context rows against a 100 000-frame map (random pooled vectors).  For L in {8, 32}, both directions,
window 50, a threshold that about 0.1 % of the entries of Q reach (read off the filtered matrix), and (sessions, paths,
min_terms) in {(1, unit, 1), (4, unit, 1), (4, unit, L / 2), (4, nine, L / 2)}, one JSON line each with the median wall
time (events around the calls, after W warm-up runs) and the peak device memory (workspaces and outputs) of
  fused_*    (a) score_session_above
  matrix_*   (b) score_all_pairs + session_filter with code + rows_above(window=-1) on the same rows: what a caller
             could do before; it has no minimum term count, so it is timed and compared at min_terms = 1 only
  seq_*      (c) score_seq_above, at one session and the unit path only: the same lists from the kernel without tables
every capacity sized to the count so that no route reads anything back.  Route (a) is checked bit for bit against
session_rows_above on the resident matrix before anything is timed, against (b) at min_terms = 1 and against (c) at one
session.  Inputs are resident.  --small: 300 x 517 and one query x 2000, 3 reps (the test suite's run)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SLOPES = ("1", "1/2", "2/3", "3/2", "2")


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
    """the value that a fraction `keep` of the finite entries of t reach"""
    flat = t.flatten()
    flat = flat[torch.isfinite(flat)]
    return float(flat.kthvalue(max(1, flat.numel() - int(flat.numel() * keep)))[0])


def same(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                  y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=4541)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--keep", type=float, default=1e-3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args(argv)
    from sg_pr_amd import engine, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    g = torch.Generator().manual_seed(1)
    if opt.small:
        opt.reps, opt.warmup, opt.map = 3, 1, 2000
        pooled_r = (torch.randn(300, eng.pw, generator=g) * 3.0).cuda()
        pooled_c = (torch.randn(517, eng.pw, generator=g) * 3.0).cuda()
    else:
        centers, labels, _, _ = synth.world_sequence(opt.graphs, 100, seed=7)
        order, cap = eng.size_order(centers, labels, 10)
        pooled_r = pooled_c = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
        eng.check_status()
    big = (torch.randn(opt.map, eng.pw, generator=g) * 3.0).cuda()
    recs = []

    def emit(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    for L in (8, 32):
        nine = engine.seq_paths(L, SLOPES)
        shapes = (("square", pooled_r, pooled_c, 0), ("one query", big[:L].contiguous(), big, L - 1))
        for name, rows, cols, ctx in shapes:
            r, m = rows.shape[0], cols.shape[0]
            for sessions, pname, paths, mt in ((1, "unit", None, 1), (4, "unit", None, 1), (4, "unit", None, L // 2),
                                               (4, "nine", nine, L // 2)):
                ct = None if sessions == 1 else np.array([(j * m) // sessions for j in range(sessions)], dtype=np.int32)
                rt = None if sessions == 1 or name != "square" else \
                    np.array([(j * r) // sessions for j in range(sessions)], dtype=np.int32)
                # (one query: the new scans and their context rows are one session, the map's last)
                row0 = 0 if name == "square" else m
                tables = dict(row_sessions=rt, col_sessions=ct)
                score = eng.score_all_pairs(rows, cols)
                q = eng.session_filter(score, L, paths, window=50, row0=row0, context=ctx, reverse="both", **tables)
                thr = value_at(q, opt.keep)
                del q
                kw = dict(min_terms=mt, window=50, row0=row0, context=ctx, reverse="both", **tables)
                want = eng.session_rows_above(score, L, thr, paths, **kw)
                del score
                n = want[0].numel()

                def fused():
                    return eng.score_session_above(rows, cols, L, thr, paths, capacity=n, **kw)

                def matrix():
                    qq, cc = eng.session_filter(eng.score_all_pairs(rows, cols), L, paths, window=50, row0=row0,
                                                context=ctx, reverse="both", want_code=True, **tables)
                    return eng.rows_above(qq, thr, window=-1, capacity=n) + (cc,)

                def seq():
                    return eng.score_seq_above(rows, cols, L, thr, window=50, row0=row0, context=ctx, reverse="both",
                                               capacity=n)

                got = fused()
                rec = {"shape": name, "rows": r, "cols": m, "context": ctx, "seq_len": L, "sessions": sessions,
                       "paths": pname, "min_terms": mt, "threshold": thr, "pairs": n,
                       "equal_resident": bool(same(got, want))}
                routes = [("fused", fused)]
                if mt == 1:
                    ref = matrix()
                    rec["equal_matrix"] = bool(same(got[:3] + (got[4],), ref[:4]) and
                                               torch.equal(got[3], ref[4][got[0].long(), got[1].long()]))
                    del ref
                    routes.append(("matrix", matrix))
                if sessions == 1 and paths is None and mt == 1:
                    rec["equal_seq"] = bool(same(got, seq()))
                    routes.append(("seq", seq))
                del got, want
                for key, fn in routes:
                    rec[key + "_ms"] = round(median_ms(fn, opt.reps, opt.warmup), 3)
                    rec[key + "_peak_mb"] = peak_mb(fn)
                if "matrix_ms" in rec:
                    rec["fused_over_matrix"] = round(rec["fused_ms"] / rec["matrix_ms"], 3)
                if "seq_ms" in rec:
                    rec["fused_over_seq"] = round(rec["fused_ms"] / rec["seq_ms"], 3)
                emit(rec)
    eng.close()
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("# python tools/session_above_bench.py --reps %d --warmup %d --keep %g%s (MI355X; times in ms, medians)\n"
                    % (opt.reps, opt.warmup, opt.keep, " --small" if opt.small else ""))
            f.write("\n".join(json.dumps(r) for r in recs) + "\n")
    return recs


if __name__ == "__main__":
    main()
