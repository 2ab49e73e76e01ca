"""Time the visibility tallies of a landmark map (sgpr_landmark_persist) on synth.landmark_world: the
search of the build, which tests every landmark, against the variant that walks a coarse cell table, and both against
the NumPy reference.

    python tools/persist_bench.py [--points 3x100,2x4541] [--reps N] [--warmup W] [--variant variants/libsgpr_NAME.so]
                                  [--ref-scans Q] [--step-timeout S] [--world-cache DIR] [--out profiles/persist.txt]

A point DxS is landmark_world with D drives of S scans.  The landmark map is built on the device from every drive but
the last at the true poses; the scans of the last drive are aligned to it from their true poses displaced by N(0, 0.02)
rad and N(0, 0.3) m (gates 2.0 then 0.75 m, landmarks with three or more observations), associated with all landmarks
(iters = 0) and folded in (landmarks.update); the call that is timed tallies that drive on the updated map with the
update's node_landmark at the defaults (range 50 m, margin 2 m, 5 expected, ratio 0.3).  Every point and library runs in
a process of its own under --step-timeout seconds (--variant: tools/build_variant.sh persist_table -DSGPR_PERSIST_SEARCH=1, run
through SGPR_HIP_LIB); a step that fails or runs out of time ends the run (nothing more is started on the device).  Per
step, one JSON line: the median of --reps calls with events around the call, the inputs resident and the workspace
allocated; the landmarks, the retired and judged ones, the median per-scan seen / expected; a sha256 over the six
outputs - the driver adds whether a variant's equals the build's -; and whether the tallies of the first --ref-scans scans
alone equal tests/landmark_persist_ref.py byte for byte.  No time is promised and none is asserted: the file records what
was measured."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUTPUTS = ("expected", "seen", "keep", "scan_stat", "view", "num")


def run_point(opt):
    import numpy as np
    import torch
    import landmark_persist_ref as ref
    from sg_pr_amd import landmarks, synth
    D, S = (int(t) for t in opt.point.split("x"))
    if D < 2:
        raise SystemExit("a point needs a map and a drive to tally: D >= 2")
    cached = os.path.join(opt.world_cache, "landmark_world_%dx%d.npz" % (D, S)) if opt.world_cache else None
    if cached and os.path.exists(cached):
        w = dict(np.load(cached))
    else:
        w = synth.landmark_world(0, scans=S, sessions=D, closures=0)
        if cached:
            os.makedirs(opt.world_cache, exist_ok=True)
            np.savez(cached, **w)
    M = (D - 1) * S
    N = w["labels"].shape[1]
    lm = landmarks.build(w["centers"][:M], w["labels"][:M], w["truth"][:M], starts=w["starts"][:D - 1])
    rng = np.random.default_rng(500)
    start = synth._se2_compose(w["truth"][M:], synth._se2(rng.normal(0, 0.02, S), rng.normal(0, 0.3, S), rng.normal(0, 0.3, S)))
    cen, lab = torch.from_numpy(w["centers"][M:]).cuda(), torch.from_numpy(w["labels"][M:]).cuda()
    X = torch.from_numpy(start).cuda()
    use = landmarks.select(lm, min_count=3)
    for r in (2.0, 0.75):
        X = landmarks.align_async(cen, lab, X, lm, use=use, radius=r, iters=10)["poses"]
    assoc = landmarks.align_async(cen, lab, X, lm, iters=0)["node_landmark"]
    up = landmarks.update(cen, lab, X, assoc, lm, session_base=D - 1, node_base=M * N)
    L = int(up["num_landmarks"])
    node = up["node_landmark"]
    ws = torch.empty(max(landmarks.persist_workspace_bytes(S, N, L), 1), dtype=torch.uint8, device="cuda")

    def call():
        return landmarks.persist_async(cen, lab, X, node, up, workspace=ws)

    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
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
    got = {k: out[k].cpu().numpy() for k in OUTPUTS}
    digest = hashlib.sha256(b"".join(np.ascontiguousarray(got[k]).tobytes() for k in OUTPUTS)).hexdigest()
    stat = got["scan_stat"]
    asked = stat[:, 0] > 0
    rec = {"point": opt.point, "library": os.path.relpath(os.environ["SGPR_HIP_LIB"], REPO) if os.environ.get("SGPR_HIP_LIB") else "in-tree",
           "scans": S, "slots": N, "landmarks": L, "in_use": int((up["count"] >= 3).sum()), "retired": int(got["num"][0]),
           "judged": int(got["num"][1]), "scans_with_view": int(got["num"][3]),
           "expected_per_scan_median": float(np.median(stat[:, 0])),
           "scan_ratio_median": float(np.median(stat[asked, 1] / stat[asked, 0])) if asked.any() else 0.0,
           "workspace_KiB": ws.numel() / 1024.0, "first_call_ms": first_ms, "call_ms": float(np.median(times)),
           "calls_ms": [round(t, 4) for t in times], "sha256": digest}
    q = min(opt.ref_scans, S)
    part = landmarks.persist_async(cen[:q], lab[:q], X[:q], node[:q], up)
    host = {"center": up["center"].cpu().numpy(), "label": up["label"].cpu().numpy()}
    t0 = time.perf_counter()
    want = ref.persist(w["centers"][M:M + q], w["labels"][M:M + q], X[:q].cpu().numpy(), node[:q].cpu().numpy(), host)
    rec["ref_scans"], rec["ref_s"] = q, time.perf_counter() - t0
    rec["equal_to_reference"] = bool(all(part[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in OUTPUTS))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default="3x100,2x4541")
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variant", action="append", default=[], help="a further library of the same C-ABI to time (repeatable)")
    ap.add_argument("--ref-scans", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--world-cache", default=None)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    if opt.point is not None:
        return run_point(opt)
    lines = ["# tools/persist_bench.py --points %s --reps %d --warmup %d --ref-scans %d%s"
             % (opt.points, opt.reps, opt.warmup, opt.ref_scans, "".join(" --variant " + v for v in opt.variant))]
    steps = [(p.strip(), lib) for p in opt.points.split(",") if p.strip() for lib in [None] + opt.variant]
    mine = {}
    for point, lib in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup", str(opt.warmup),
               "--ref-scans", str(opt.ref_scans)] + (["--world-cache", opt.world_cache] if opt.world_cache else [])
        env = dict(os.environ)
        env.pop("SGPR_HIP_LIB", None)
        if lib is not None:
            env["SGPR_HIP_LIB"] = os.path.abspath(lib)
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.step_timeout, env=env)
        except subprocess.TimeoutExpired:
            print("point %s (%s) ran out of time: stopping" % (point, lib or "in-tree"), flush=True)
            break
        final = [t for t in done.stdout.splitlines() if t.startswith("{")]
        if done.returncode != 0 or not final:
            sys.stdout.write(done.stdout[-2000:])
            print("point %s (%s) failed with status %d: stopping" % (point, lib or "in-tree", done.returncode), flush=True)
            break
        rec = json.loads(final[-1])
        if lib is None:
            mine[point] = rec
        else:
            rec["equal_to_in_tree"] = rec["sha256"] == mine[point]["sha256"]
            rec["over_in_tree"] = rec["call_ms"] / mine[point]["call_ms"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(lines) == 1 + len(steps) else 1


if __name__ == "__main__":
    sys.exit(main())
