"""Time the planar pose-graph relaxation (sgpr_posegraph_optimize) on synth.drift_world.

    python tools/posegraph_bench.py [--points 2x300,3x1500,5x4541] [--reps N] [--warmup W] [--ref-max M]
                                    [--step-timeout S] [--out profiles/posegraph.txt]

A point SxN is a map of S sessions of N scans with S N / 10 closures (120 at 2x300, the default world of the tests).
Every point runs in a process of its own under --step-timeout seconds; a point that fails or runs out of time ends the
run (nothing more is started on the device).  Per point, one JSON line: the median wall time of the call (events around
it; the call is one kernel), the iterations of the two stages and the time per iteration, the merged-map trajectory
error before and after and the per-session odometry error, the time of a direct solve of the same two normal equations
on the host (scipy.sparse.linalg.spsolve on tests/posegraph_ref.py's assembly; the assembly is timed apart) and the
largest gap between the two solutions, and - up to --ref-max scans - the NumPy reference's time and whether the GPU
result equals it bit for bit.  No speed is gated on: the file records what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def run_point(opt):
    import numpy as np
    import scipy.sparse.linalg
    import torch
    import posegraph_ref as ref
    from sg_pr_amd import metrics, posegraph, synth
    sessions, scans = (int(t) for t in opt.point.split("x"))
    M = sessions * scans
    C = 120 if M == 600 else M // 10
    w = synth.drift_world(0, scans=scans, sessions=sessions, closures=C)
    X, T = torch.from_numpy(w["odom"]).cuda(), torch.from_numpy(w["T"]).cuda()
    rows, cols = torch.from_numpy(w["rows"]).cuda(), torch.from_numpy(w["cols"]).cuda()
    ws = torch.empty(posegraph.workspace_bytes(M, C), dtype=torch.uint8, device="cuda")
    kw = dict(starts=w["starts"], max_iters=opt.max_iters, rel_tol=opt.rel_tol)

    def call():
        return posegraph.optimize_async(X, rows, cols, T, workspace=ws, **kw)

    t0 = time.perf_counter()
    out, info, resid = call()
    torch.cuda.synchronize()
    rec = {"point": opt.point, "M": M, "C": C, "rel_tol": opt.rel_tol, "first_call_ms": 1e3 * (time.perf_counter() - t0)}
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
    d = posegraph.info_dict(info.cpu().numpy(), resid.cpu().numpy())
    its = sum(d["iterations"])
    rec.update({"call_ms": float(np.median(times)), "iterations": list(d["iterations"]), "stop": list(d["stop"]),
                "us_per_iteration": 1e3 * float(np.median(times)) / max(its, 1), "status": d["status"],
                "live_closures": d["live_closures"], "free_scans": d["free_scans"]})
    got = out.cpu().numpy()
    per = metrics.trajectory_error(w["odom"], w["truth"], w["starts"])
    rec.update({"error_before_m": metrics.trajectory_error(w["odom"], w["truth"]),
                "error_after_m": metrics.trajectory_error(got, w["truth"]),
                "odometry_error_per_session_rms_m": float(np.sqrt(np.mean(per ** 2)))})
    print(json.dumps({"point": opt.point, "progress": "device timed", "call_ms": rec["call_ms"]}), flush=True)
    t0 = time.perf_counter()
    solve = ref.normal_equations(w["odom"], w["rows"], w["cols"], w["T"], starts=w["starts"])
    rec["host_assembly_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    direct = solve(scipy.sparse.linalg.spsolve)
    rec["host_spsolve_s"] = time.perf_counter() - t0
    rec["gap_to_direct"] = float(np.abs(got - direct).max())
    if M <= opt.ref_max:
        t0 = time.perf_counter()
        want = ref.optimize(w["odom"], w["rows"], w["cols"], w["T"], **kw)
        rec["ref_s"] = time.perf_counter() - t0
        rec["equal_to_reference"] = bool(got.tobytes() == want[0].tobytes() and
                                         np.array_equal(info.cpu().numpy(), want[1]) and
                                         resid.cpu().numpy().tobytes() == want[2].tobytes())
    else:
        rec["ref_skipped"] = "M above --ref-max %d" % opt.ref_max
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="2x300,3x1500,5x4541")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--rel-tol", type=float, default=1e-9)
    ap.add_argument("--ref-max", type=int, default=4500, help="largest map the NumPy reference is run at")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per point")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    if opt.point is not None:
        return run_point(opt)
    lines = []
    for point in [t.strip() for t in opt.points.split(",") if t.strip()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup",
               str(opt.warmup), "--max-iters", str(opt.max_iters), "--rel-tol", repr(opt.rel_tol), "--ref-max", str(opt.ref_max)]
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
            f.write("# tools/posegraph_bench.py --points %s --reps %d --warmup %d --max-iters %d --rel-tol %g\n"
                    % (opt.points, opt.reps, opt.warmup, opt.max_iters, opt.rel_tol))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
