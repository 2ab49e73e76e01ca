"""Time scan localisation (sgpr_localize_scans) on synth.localize_world beside the NumPy reference.

    python tools/localize_bench.py [--points 200x8x8,4541x32x8,4541x64x16] [--reps N] [--warmup W] [--ref-queries R]
                                   [--step-timeout S] [--out profiles/localize.txt]

A point QxKxL is localize_world scaled up: a map of 3 Q scans, Q queries with K candidates each, the last L scans voting.
Every point runs in a process of its own under --step-timeout seconds; a point that fails or runs out of time ends the
run (nothing more is started on the device).  Per point, one JSON line: the median wall time of the call (events around
it; the call is one kernel) with the inputs already on the device, the pair tests per second that makes (Q (L K)^2), the
share of queries with a support of at least 5 and the share of those within 1 m of the truth, the time of the NumPy
reference (tests/localize_ref.py) on the host and whether the device result equals it bit for bit.  Where Q (L K)^2
exceeds 1e9 the reference answers --ref-queries evenly spaced queries only (a query's answer does not depend on which
others are asked) and its time for all Q is extrapolated from those; the line says so.  No speed is gated on: the file
records what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def same(got, want):
    import numpy as np
    if got.dtype.kind != "f":
        return bool((got == want).all())
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all()) and np.where(gn, 0.0, got).tobytes() == np.where(wn, 0.0, want).tobytes()


def run_point(opt):
    import numpy as np
    import torch
    import localize_ref as ref
    from sg_pr_amd import localize, metrics, synth
    Q, K, L = (int(t) for t in opt.point.split("x"))
    w = synth.localize_world(0, map_scans=3 * Q, queries=Q, k=K)
    dev = {name: torch.from_numpy(w[name]).cuda() for name in ("map", "cols", "T", "odom")}

    def call():
        return localize.localize_async(dev["map"], dev["cols"], dev["T"], odo=dev["odom"] if L > 1 else None, seq_len=L)

    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    rec = {"point": opt.point, "Q": Q, "K": K, "L": L, "first_call_ms": 1e3 * (time.perf_counter() - t0)}
    for _ in range(opt.warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(opt.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    pose, stat, spread = (t.cpu().numpy() for t in out)
    tests = float(Q) * (L * K) ** 2
    acc = stat[:, 0] >= 5
    err = metrics.localization_errors(pose, w["truth"])["trans_m"]
    rec.update({"call_ms": float(np.median(times)), "pair_tests": tests,
                "pair_tests_per_s": tests / (1e-3 * float(np.median(times))), "accepted_support_5": float(acc.mean()),
                "accepted_within_1m": float((err[acc] <= 1.0).mean()) if acc.any() else None})
    print(json.dumps({"point": opt.point, "progress": "device timed", "call_ms": rec["call_ms"]}), flush=True)
    only = None if tests <= 1e9 else np.unique(np.linspace(0, Q - 1, min(opt.ref_queries, Q)).astype(np.int64))
    t0 = time.perf_counter()
    want = ref.localize(w["map"], w["cols"], w["T"], odo=w["odom"] if L > 1 else None, L=L, only=only)
    took = time.perf_counter() - t0
    rows = slice(None) if only is None else only
    rec["equal_to_reference"] = bool(same(pose[rows], want[0][rows]) and same(stat[rows], want[1][rows]) and
                                     same(spread[rows], want[2][rows]))
    if only is None:
        rec["ref_s"] = took
    else:
        rec.update({"ref_queries": int(only.size), "ref_s_for_those": took, "ref_s_extrapolated": took * Q / only.size})
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="200x8x8,4541x32x8,4541x64x16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-queries", type=int, default=128, help="queries the reference answers at the large points")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per point")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    if opt.point is not None:
        return run_point(opt)
    lines = []
    for point in [t.strip() for t in opt.points.split(",") if t.strip()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup",
               str(opt.warmup), "--ref-queries", str(opt.ref_queries)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.step_timeout)
        except subprocess.TimeoutExpired as e:
            tail = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            lines.append(json.dumps({"point": point, "error": "ran past the step limit of %g s; nothing more is started"
                                     % opt.step_timeout, "output": tail[-400:]}))
            print(lines[-1], flush=True)
            break
        final = [ln for ln in done.stdout.splitlines() if ln.startswith("{") and '"progress"' not in ln]
        if done.returncode != 0 or not final:
            lines.append(json.dumps({"point": point, "error": "exit status %d; nothing more is started" % done.returncode,
                                     "output": done.stdout[-400:]}))
            print(lines[-1], flush=True)
            break
        lines.append(final[-1])
        print(final[-1], flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("# tools/localize_bench.py --points %s --reps %d --warmup %d --ref-queries %d\n"
                    % (opt.points, opt.reps, opt.warmup, opt.ref_queries))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
