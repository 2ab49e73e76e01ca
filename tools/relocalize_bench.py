"""Time the relocalisation of scans in a landmark map (sgpr_landmark_relocalize) on synth.landmark_world.

    python tools/relocalize_bench.py [--points 300,4541] [--reps 10] [--warmup 2] [--ref-scans Q] [--step-timeout S]
                                     [--out profiles/relocalize.txt]

A point S is landmark_world(0, scans=S) with three drives: the landmark map is built on the device from drives 0 and 1
at the true poses, its landmarks with three or more observations are in use, and EVERY scan of drive 2 is a query of one
call - no pose goes in.  The defaults of landmarks.relocalize: inlier gate 0.75 m, refine gates 2.0 and 0.75 m, 10
iterations, base pairs 5..30 m, tau_edge 0.5, max_hyp 65536, min_inliers 12, sep 10 m.  Every point runs in a process of
its own under --step-timeout seconds; a point that fails or runs out of time ends the run (nothing more is started on
the device).  Per point, one JSON line: the median of --reps calls after --warmup calls, events around the call, the
inputs resident and the workspace allocated; microseconds per scan; the median and the largest number of hypotheses of
a scan; the share of scans found, found within 0.5 m of the truth, ambiguous and truncated; tests/landmark_relocalize_ref.py
on the first --ref-scans scans and whether the call equals it there.  No time is promised and none is asserted: the
file records what was measured."""
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
    import torch
    import landmark_relocalize_ref as ref
    from sg_pr_amd import landmarks, synth
    S = int(opt.point)
    w = synth.landmark_world(0, scans=S, closures=0)
    M = 2 * S
    lm = landmarks.build(w["centers"][:M], w["labels"][:M], w["truth"][:M], starts=w["starts"][:2])
    use = landmarks.select(lm, min_count=3)
    truth = w["truth"][M:]
    host = {"centers": w["centers"][M:], "labels": w["labels"][M:]}
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    Q, N = host["labels"].shape
    L = int(lm["num_landmarks"])
    ws = torch.empty(max(landmarks.relocalize_workspace_bytes(Q, N, L, 2), 1), dtype=torch.uint8, device="cuda")

    def call():
        return landmarks.relocalize_async(dev["centers"], dev["labels"], lm, use=use, workspace=ws)

    out = call()
    torch.cuda.synchronize()
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
    got = {k: v.cpu().numpy() for k, v in out.items()}
    st = got["stat"]
    found = (st[:, 5] & landmarks.RELOC_FOUND) != 0
    err = np.hypot(got["poses"][:, 2] - truth[:, 2], got["poses"][:, 3] - truth[:, 3])
    amb = found & (st[:, 1] >= 0.7 * st[:, 0])
    rec = {"point": opt.point, "queries": Q, "slots": N, "landmarks": L, "in_use": int(use.sum()),
           "call_ms": float(np.median(times)), "calls_ms": [round(t, 3) for t in times],
           "call_us_per_scan": 1000.0 * float(np.median(times)) / Q, "workspace_KiB": ws.numel() / 1024.0,
           "hypotheses_median": float(np.median(got["hypotheses"])), "hypotheses_max": int(got["hypotheses"].max()),
           "found": float(found.mean()), "found_within_0.5m": float((found & (err < 0.5)).mean()), "ambiguous": float(amb.mean()),
           "truncated": float(((st[:, 5] & landmarks.RELOC_TRUNCATED) != 0).mean()), "num": got["num"].tolist(),
           "median_error_m": float(np.median(err[found])) if found.any() else None,
           "max_error_m": float(err[found].max()) if found.any() else None,
           "inliers_median": float(np.median(st[:, 0])), "inliers_other_max": int(st[:, 1].max())}
    if opt.ref_scans > 0:
        n = min(Q, opt.ref_scans)
        t0 = time.perf_counter()
        want = ref.relocalize(host["centers"][:n], host["labels"][:n], lm["center"].cpu().numpy(), lm["label"].cpu().numpy(),
                              use.cpu().numpy())
        rec["ref_scans"] = n
        rec["ref_s"] = time.perf_counter() - t0
        rec["equal_to_reference"] = bool(all(got[k][:n].tobytes() == want[r].tobytes() for k, r in (
            ("poses", "poses"), ("coarse", "coarse"), ("other", "other"), ("node_landmark", "node_landmark"), ("stat", "stat"),
            ("win", "win"), ("hypotheses", "hyp"), ("rms", "rms"))))
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="300,4541")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-scans", type=int, default=30, help="scans the NumPy reference is run and compared on")
    ap.add_argument("--step-timeout", type=float, default=420.0, help="seconds per point")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    if opt.point is not None:
        return run_point(opt)
    lines = []
    for point in [t.strip() for t in opt.points.split(",") if t.strip()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup", str(opt.warmup),
               "--ref-scans", str(opt.ref_scans)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"point": point, "error": "ran past the step limit of %g s; nothing more is started" % opt.step_timeout}))
            print(lines[-1], flush=True)
            break
        final = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode != 0 or not final:
            lines.append(json.dumps({"point": point, "error": "exit status %d; nothing more is started" % done.returncode,
                                     "output": done.stdout[-400:]}))
            print(lines[-1], flush=True)
            break
        lines.append(final[-1])
        print(final[-1], flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("# tools/relocalize_bench.py --points %s --reps %d --warmup %d --ref-scans %d\n"
                    % (opt.points, opt.reps, opt.warmup, opt.ref_scans))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
