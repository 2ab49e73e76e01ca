"""What session tables cost and what they find: sgpr_score_session_topk beside sgpr_score_path_topk at equal arguments.

    python tools/session_bench.py [--reps N] [--warmup W] [--out profiles/session_bench.txt] [--tiny]

One process, inputs resident.  synth.world_sequence(4541, 100) against itself, window 50, both directions.
  time        L in {8, 16}, k in {1, 16}, the unit path and the 9-path set {1, 1/2, 2/3, 3/2, 2}: path_ms
              (score_path_topk, radius 0), session1_ms (score_session_topk with one session: the same lists) and
              session4_ms (four equal sessions, rows and columns) - median wall time of one call, events around the
              call, after W warm-up calls -, the ratios session1_over_path (expected near 1.0: the inner loop is the
              path kernel's) and session4_over_path (reported only), and the peak device memory of the three calls.
  recall      the lists of `python -m sg_pr_amd.place_db --sessions 4`: recall@1 / recall@k of the session lists beside
              the one-trajectory lists, over all rows and over the head rows (fewer than 50 scans after the start of a
              session with a predecessor), all under the session rule for an allowed match.
--tiny: 240 scans, 2 repetitions (a smoke run; writes no file unless --out is given)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from path_bench import SLOPES, median_ms, peak_mb   # noqa: E402

LENGTHS, KS, WINDOW, SESSIONS = (8, 16), (1, 16), 50, 4


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
        opt.out = os.path.join(REPO, "profiles", "session_bench.txt")
    from sg_pr_amd import engine, metrics, synth
    from oracle import sgpr_oracle
    eng = engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")), device=0)
    centers, labels, _, poses = synth.world_sequence(opt.graphs, 100)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    eng.check_status()
    n = opt.graphs
    one = np.zeros(1, dtype=np.int32)
    four = np.array([(j * n) // SESSIONS for j in range(SESSIONS)], dtype=np.int32)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for L in LENGTHS:
        for name, paths in (("unit", engine.seq_paths(L, ["1"])), ("nine", engine.seq_paths(L, SLOPES))):
            for k in KS:
                def path():
                    return eng.score_path_topk(pooled, pooled, L, paths, k=k, window=WINDOW)

                def sess1():
                    return eng.score_session_topk(pooled, pooled, L, paths, row_sessions=one, col_sessions=one, k=k,
                                                  window=WINDOW)

                def sess4():
                    return eng.score_session_topk(pooled, pooled, L, paths, row_sessions=four, col_sessions=four, k=k,
                                                  window=WINDOW)
                same = all(torch.equal(a, b) for a, b in zip(path(), sess1()))     # one session: the same lists
                p_ms, s1_ms, s4_ms = (median_ms(f, opt.reps, opt.warmup) for f in (path, sess1, sess4))
                emit({"rows": n, "cols": n, "seq_len": L, "k": k, "paths": int(paths.shape[0]), "path_set": name,
                      "path_ms": round(p_ms, 3), "session1_ms": round(s1_ms, 3), "session4_ms": round(s4_ms, 3),
                      "session1_over_path": round(s1_ms / p_ms, 3), "session4_over_path": round(s4_ms / p_ms, 3),
                      "one_session_lists_equal": bool(same), "path_peak_mb": round(peak_mb(path), 1),
                      "session1_peak_mb": round(peak_mb(sess1), 1), "session4_peak_mb": round(peak_mb(sess4), 1)})
    frames = np.arange(n)
    head = np.zeros(n, dtype=bool)
    for s0 in four[1:]:
        head |= (frames >= s0) & (frames < s0 + WINDOW)
    for L in LENGTHS:
        for k in KS:
            plain = eng.score_seq_topk(pooled, pooled, L, k=k, window=WINDOW)[1]
            sess = eng.score_session_topk(pooled, pooled, L, None, row_sessions=four, col_sessions=four, k=k,
                                          window=WINDOW)[1]
            kw = dict(p_thresh=3.0, window=WINDOW, col_starts=four)
            rec = {"sessions": SESSIONS, "seq_len": L, "k": k, "head_rows": int(head.sum())}
            for what, mask in (("all", None), ("head", head)):
                a = metrics.recall_at_n(sess, poses, row_mask=mask, **kw)
                b = metrics.recall_at_n(plain, poses, row_mask=mask, **kw)
                rec.update({"recall1_%s" % what: round(float(a[0]), 4), "recall1_%s_one_trajectory" % what: round(float(b[0]), 4),
                            "recallk_%s" % what: round(float(a[-1]), 4),
                            "recallk_%s_one_trajectory" % what: round(float(b[-1]), 4)})
            emit(rec)
    eng.close()
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("# python tools/session_bench.py --reps %d --warmup %d --graphs %d (MI355X; times in ms, medians)\n"
                    % (opt.reps, opt.warmup, opt.graphs))
            f.write("\n".join(json.dumps(r) for r in records) + "\n")
    return records


if __name__ == "__main__":
    main()
