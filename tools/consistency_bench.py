"""Time pairwise-consistent closure selection (sgpr_closure_consistency, sgpr_consistent_set) on the planted
world of synth.closure_world.

    python tools/consistency_bench.py [--points 400,4096,16384] [--outlier-frac F] [--reps N] [--warmup W]
                                      [--step-timeout S] [--out profiles/consistency.txt]

Every point runs in a process of its own under --step-timeout seconds; a point that fails or runs out of time ends the
run (nothing more is started on the device).  Per point, one JSON line: the median wall time of each of the two calls
(events around the call), the time of each of the three kernels inside them (torch.profiler's device activity, by kernel
name; absent if the profiler reports none), the NumPy reference's time on the same input (tests/consistency_ref.py) and
whether the GPU results equal it, the clique sizes, and the precision of the closures before and after the selection.
Before a point larger than the last one measured, the clique kernel's time is bounded from that one: one group runs in
ONE workgroup, and even if every round recounted every candidate (C^2 ceil(C/64) word operations for a set that holds a
fixed share of C) the time would grow with the cube of C; if that many calls at that bound would take more than half
the step's time limit, the point runs without the clique and says so.  No speed is gated on: the file records what was measured."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
KERNELS = ("cc_prep_kernel", "cc_pair_kernel", "cs_clique_kernel")


def median_ms(fn, reps, warmup):
    import numpy as np
    import torch
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


def kernel_ms(fn):
    """device time of each of the three kernels in one run of fn, by name (torch.profiler) -> dict, empty if none seen"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for name in KERNELS:
                if name in ev.name:
                    dur = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    out[name + "_ms"] = out.get(name + "_ms", 0.0) + dur / 1e3
        return out
    except Exception as e:      # a profiler that cannot attach is not a reason to lose the wall times
        return {"profiler_error": repr(e)[:200]}


def run_point(opt):
    import numpy as np
    import torch
    import consistency_ref as ref
    from sg_pr_amd import engine, synth
    C = int(opt.point)
    w = synth.closure_world(0, scans=600, closures=C, outlier_frac=opt.outlier_frac)
    tol = (1.0, math.cos(0.06), 0.04)
    group = np.zeros(C, np.int32)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], group)]
    rec = {"C": C, "outlier_frac": opt.outlier_frac, "planted": int(w["planted"].sum()), "aliased": int(w["aliased"].sum())}

    def consistency():
        return engine.closure_consistency(*dev, 1, *tol)

    adj, degree, members = consistency()
    torch.cuda.synchronize()
    rec["consistency_ms"] = median_ms(consistency, opt.reps, opt.warmup)
    rec.update(kernel_ms(consistency))
    print(json.dumps({"C": C, "progress": "consistency timed", "consistency_ms": rec["consistency_ms"]}), flush=True)
    rank = size = None
    if not opt.no_clique:
        def clique():
            return engine.consistent_set(adj, members, 1)

        t0 = time.perf_counter()
        rank, size = clique()
        torch.cuda.synchronize()
        rec["clique_first_call_ms"] = 1e3 * (time.perf_counter() - t0)
        rec["clique_ms"] = median_ms(clique, opt.reps, opt.warmup)
        rec.update(kernel_ms(clique))
        print(json.dumps({"C": C, "progress": "clique timed", "clique_ms": rec["clique_ms"]}), flush=True)
    else:
        rec["clique_skipped"] = opt.no_clique
    if C <= opt.ref_max:
        t0 = time.perf_counter()
        w_adj, w_degree, w_members = ref.closure_consistency(w["rows"], w["cols"], w["T"], w["Xr"], w["Xc"], group, 1, *tol)
        rec["ref_consistency_s"] = time.perf_counter() - t0
        print(json.dumps({"C": C, "progress": "reference matrix done", "s": rec["ref_consistency_s"]}), flush=True)
        t0 = time.perf_counter()
        w_rank, w_size = ref.consistent_set(w_adj, w_members, 1)
        rec["ref_clique_s"] = time.perf_counter() - t0
        rec["equal_matrix"] = bool(np.array_equal(adj.cpu().numpy(), w_adj) and np.array_equal(degree.cpu().numpy(), w_degree))
        if rank is not None:
            rec["equal_clique"] = bool(np.array_equal(rank.cpu().numpy(), w_rank) and np.array_equal(size.cpu().numpy(), w_size))
        else:
            rank, size = torch.from_numpy(w_rank), torch.from_numpy(w_size)
            rec["clique_from"] = "reference"
    else:
        rec["ref_skipped"] = "C above --ref-max %d" % opt.ref_max
    deg = degree.cpu().numpy()
    rec["precision_before"] = float(w["planted"].mean())
    rec["support10_accepts_aliased"] = int(((deg >= 10) & w["aliased"]).sum())
    if rank is not None:
        sel = rank.cpu().numpy() >= 0
        rec["clique_size"] = int(size[0])
        rec["selected_planted"] = int((sel & w["planted"]).sum())
        rec["selected_aliased"] = int((sel & w["aliased"]).sum())
        rec["precision_after"] = float((sel & w["planted"]).sum() / max(int(sel.sum()), 1))
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="400,4096,16384")
    ap.add_argument("--outlier-frac", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds per point")
    ap.add_argument("--ref-max", type=int, default=16384, help="largest C the NumPy reference is run at")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-clique", default="", help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    if opt.point is not None:
        return run_point(opt)
    lines, last = [], None
    for C in [int(t) for t in opt.points.split(",") if t.strip()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", str(C), "--outlier-frac", str(opt.outlier_frac),
               "--reps", str(opt.reps), "--warmup", str(opt.warmup), "--ref-max", str(opt.ref_max)]
        if last is not None and "clique_ms" in last and C > last["C"]:
            est = last["clique_ms"] * (C / last["C"]) ** 3
            note = "clique kernel bounded at %.0f ms per call from C = %d (%.2f ms, cube of C)" % (est, last["C"], last["clique_ms"])
            if est * (opt.reps + opt.warmup + 2) > 500.0 * opt.step_timeout:
                note += ": more than half of the %g s step limit for %d calls, the point runs without it" % (
                    opt.step_timeout, opt.reps + opt.warmup + 2)
                cmd += ["--no-clique", note]
            lines.append(json.dumps({"C": C, "note": note}))
            print(lines[-1], flush=True)
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.step_timeout)
        except subprocess.TimeoutExpired as e:
            lines.append(json.dumps({"C": C, "error": "ran past the step limit of %g s; nothing more is started" % opt.step_timeout,
                                     "output": (e.stdout or b"").decode(errors="replace")[-400:] if isinstance(e.stdout, bytes)
                                     else (e.stdout or "")[-400:]}))
            print(lines[-1], flush=True)
            break
        final = [ln for ln in done.stdout.splitlines() if ln.startswith("{") and '"progress"' not in ln]
        if done.returncode != 0 or not final:
            lines.append(json.dumps({"C": C, "error": "exit status %d; nothing more is started" % done.returncode,
                                     "output": done.stdout[-400:]}))
            print(lines[-1], flush=True)
            break
        last = json.loads(final[-1])
        lines.append(final[-1])
        print(final[-1], flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("# tools/consistency_bench.py --points %s --outlier-frac %g --reps %d --warmup %d\n"
                    % (opt.points, opt.outlier_frac, opt.reps, opt.warmup))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
