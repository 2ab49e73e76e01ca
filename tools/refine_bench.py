"""Time the landmark refinement (sgpr_landmark_refine) on synth.landmark_world beside its NumPy reference.

    python tools/refine_bench.py [--points 1x600,1x4541,5x4541] [--iters T] [--reps N] [--warmup W] [--ref-nodes P]
                                 [--step-timeout S] [--out profiles/refine.txt]

A point DxS is landmark_world with D drives of S scans; the poses are the true ones with every scan displaced by
N(0, 0.004) rad and N(0, 0.03) m, the landmark map is built on them on the device (landmarks.build) and the landmarks with
two or more observations take part, scan 0 fixed.  Every point runs in a process of its own under --step-timeout seconds; a
point that fails or runs out of time ends the run (nothing more is started on the device).  Per point, one JSON line: the
median wall time of the call (events around it) with the inputs already on the device and the workspace allocated, nodes,
landmarks, launches, the cost before and after.  The host column is the NumPy reference (tests/landmark_refine_ref.py),
once, on the same inputs, when the point has at most --ref-nodes node slots; there poses, costs and info are compared bit
for bit; elsewhere the line says that they were not.  No speed is gated on: the file records what was measured, the case
where the host is faster included."""
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
    import landmark_refine_ref as ref
    from sg_pr_amd import engine, landmarks, synth
    D, S = (int(t) for t in opt.point.split("x"))
    w = synth.landmark_world(0, scans=S, sessions=D, closures=0)
    G, N = w["labels"].shape
    rng = np.random.default_rng(50)
    start = synth._se2_compose(w["truth"], synth._se2(rng.normal(0, 0.004, G), rng.normal(0, 0.03, G), rng.normal(0, 0.03, G)))
    dev = {name: torch.from_numpy(np.ascontiguousarray(v)).cuda() for name, v in
           (("centers", w["centers"]), ("labels", w["labels"]), ("poses", start))}
    lm = landmarks.build(dev["centers"], dev["labels"], dev["poses"], starts=w["starts"])
    use = landmarks.select(lm, min_count=2).to(torch.uint8)
    fixed = torch.zeros(G, dtype=torch.uint8, device="cuda")
    fixed[0] = 1
    L = lm["num_landmarks"]
    ws = torch.empty(max(landmarks.refine_workspace_bytes(G, N, L), 1), dtype=torch.uint8, device="cuda")

    def call():
        return landmarks.refine_async(dev["centers"], dev["labels"], dev["poses"], lm, use=use, fixed=fixed, iters=opt.iters,
                                      workspace=ws)

    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    rec = {"point": opt.point, "library": os.path.basename(os.path.dirname(engine.load_library()._name)) + "/" +
           os.path.basename(engine.load_library()._name), "scans": G, "slots": N, "landmarks": L, "iters": opt.iters,
           "launches": 2 * opt.iters + 4, "workspace_MiB": ws.numel() / 2.0 ** 20, "first_call_ms": 1e3 * (time.perf_counter() - t0)}
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
    ms = float(np.median(times))
    rec.update({"call_ms": ms, "used_nodes": int(got["info"][0]), "landmarks_observed": int(got["info"][1]),
                "refitted": int(got["info"][2]), "kept_free": int(got["info"][3]), "cost_first": float(got["cost"][0]),
                "cost_last": float(got["cost"][-1]), "node_steps_per_s": int(got["info"][0]) * (opt.iters + 1) / (1e-3 * ms)})
    print(json.dumps({"point": opt.point, "progress": "device timed", "call_ms": ms}), flush=True)
    if G * N > opt.ref_nodes:
        rec["ref_s"] = "not measured: %d node slots exceed --ref-nodes %d" % (G * N, opt.ref_nodes)
        rec["equal_to_reference"] = "not checked: the reference was not run"
    else:
        t0 = time.perf_counter()
        want = ref.refine(w["centers"], lm["node_landmark"].cpu().numpy(), start, use.cpu().numpy(), fixed=fixed.cpu().numpy(),
                          iters=opt.iters)
        rec["ref_s"] = time.perf_counter() - t0
        rec["equal_to_reference"] = bool(got["poses"].tobytes() == want["poses"].tobytes() and
                                         got["cost"].tobytes() == want["cost"].tobytes() and
                                         got["info"].tolist() == want["info"].tolist())
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x600,1x4541,5x4541")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-nodes", type=int, default=4000000, help="node slots the NumPy reference is run on at most")
    ap.add_argument("--step-timeout", type=float, default=400.0, help="seconds per point")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    if opt.point is not None:
        return run_point(opt)
    lines = []
    for point in [t.strip() for t in opt.points.split(",") if t.strip()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--iters", str(opt.iters), "--reps", str(opt.reps),
               "--warmup", str(opt.warmup), "--ref-nodes", str(opt.ref_nodes)]
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
            f.write("# tools/refine_bench.py --points %s --iters %d --reps %d --warmup %d --ref-nodes %d\n"
                    % (opt.points, opt.iters, opt.reps, opt.warmup, opt.ref_nodes))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
