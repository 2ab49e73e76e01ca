"""Time the alignment of scans to a landmark map (sgpr_landmark_align) on synth.landmark_world.

    python tools/align_bench.py [--points 3x100,1x600,1x4541,5x4541] [--iters T] [--radius R] [--reps N] [--warmup W]
                                [--variant variants/libsgpr_NAME.so] [--ref-scans Q] [--step-timeout S]
                                [--world-cache DIR] [--out profiles/align.txt]

A point DxS is landmark_world with D drives of S scans.  The landmark map is built on the device from every drive but
the last at the true poses (a single drive: from that drive itself, and the map then contains the queries), its
landmarks with three or more observations are in use (one drive: two or more), and the scans of the last drive are
aligned from their true poses displaced by N(0, 0.02) rad and N(0, 0.3) m.  Every point runs in a process of its own
under --step-timeout seconds; a point that fails or runs out of time ends the run (nothing more is started on the
device).  Per point, one JSON line: the median of --reps calls with events around the call, the inputs resident and the
workspace allocated; the same for the library given by --variant (tools/build_variant.sh NAME -DSGPR_ALIGN_SEARCH=1
forces the cell table, =2 the test of every landmark), loaded in a further process of its own, when one is given;
tests/landmark_align_ref.py timed once on the first --ref-scans queries (the scans are independent, so their outputs are
comparable on their own) and whether every output of those scans is equal to it bit for bit; the errors before and
after.  --world-cache DIR keeps every generated world in DIR, so that the libraries of a point share one.  No time is
promised and none is asserted: the file records what was measured."""
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
    import landmark_align_ref as ref
    from sg_pr_amd import landmarks, synth
    D, S = (int(t) for t in opt.point.split("x"))
    cached = os.path.join(opt.world_cache, "landmark_world_%dx%d.npz" % (D, S)) if opt.world_cache else None
    if cached and os.path.exists(cached):
        w = dict(np.load(cached))
    else:
        w = synth.landmark_world(0, scans=S, sessions=D, closures=0)
        if cached:
            os.makedirs(opt.world_cache, exist_ok=True)
            np.savez(cached, **w)
    M = (D - 1) * S if D > 1 else S
    lm = landmarks.build(w["centers"][:M], w["labels"][:M], w["truth"][:M], starts=w["starts"][:max(D - 1, 1)])
    use = landmarks.select(lm, min_count=3 if D > 1 else 2)
    q0 = (D - 1) * S
    rng = np.random.default_rng(500)
    Q, N = w["labels"][q0:].shape
    truth = w["truth"][q0:]
    start = synth._se2_compose(truth, synth._se2(rng.normal(0, 0.02, Q), rng.normal(0, 0.3, Q), rng.normal(0, 0.3, Q)))
    dev = {"centers": torch.from_numpy(w["centers"][q0:]).cuda(), "labels": torch.from_numpy(w["labels"][q0:]).cuda(),
           "start": torch.from_numpy(start).cuda()}
    L = int(lm["num_landmarks"])
    ws = torch.empty(max(landmarks.align_workspace_bytes(Q, N, L), 1), dtype=torch.uint8, device="cuda")

    def call():
        return landmarks.align_async(dev["centers"], dev["labels"], dev["start"], lm, use=use, radius=opt.radius,
                                     iters=opt.iters, workspace=ws)

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

    def err(X):
        return np.hypot(X[:, 2] - truth[:, 2], X[:, 3] - truth[:, 3])
    rec = {"point": opt.point, "library": os.path.relpath(os.environ["SGPR_HIP_LIB"], REPO) if os.environ.get("SGPR_HIP_LIB") else "in-tree", "queries": Q, "slots": N, "landmarks": L,
           "in_use": int(use.sum()), "iters": opt.iters, "radius": opt.radius, "call_ms": float(np.median(times)),
           "calls_ms": [round(t, 4) for t in times], "workspace_KiB": ws.numel() / 1024.0,
           "median_error_before_m": float(np.median(err(start))), "median_error_after_m": float(np.median(err(got["poses"]))),
           "matched": int(got["stat"][:, 0].sum()), "live": int(got["stat"][:, 1].sum())}
    if not opt.no_ref:
        n = min(Q, opt.ref_scans)
        t0 = time.perf_counter()
        want = ref.align(w["centers"][q0:q0 + n], w["labels"][q0:q0 + n], start[:n], lm["center"].cpu().numpy(),
                         lm["label"].cpu().numpy(), lm_use=use.cpu().numpy(), radius=opt.radius, iters=opt.iters)
        rec["ref_scans"] = n
        rec["ref_s"] = time.perf_counter() - t0
        rec["equal_to_reference"] = bool(all(got[k][:n].tobytes() == want[k].tobytes() for k in want))
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="3x100,1x600,1x4541,5x4541")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--radius", type=float, default=0.75)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variant", action="append", default=[], help="a further library of the same C-ABI to time (repeatable)")
    ap.add_argument("--ref-scans", type=int, default=200, help="queries the NumPy reference is run and compared on")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per point and library")
    ap.add_argument("--world-cache", default=None, help="a directory that keeps the generated worlds between processes")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-ref", action="store_true", help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    if opt.point is not None:
        return run_point(opt)
    lines = []

    def step(point, lib):
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--iters", str(opt.iters), "--radius", str(opt.radius),
               "--reps", str(opt.reps), "--warmup", str(opt.warmup), "--ref-scans", str(opt.ref_scans)]
        if opt.world_cache:
            cmd += ["--world-cache", opt.world_cache]
        env = dict(os.environ)
        env.pop("SGPR_HIP_LIB", None)
        if lib is not None:
            env["SGPR_HIP_LIB"] = os.path.abspath(lib)
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.step_timeout, env=env)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"point": point, "library": lib or "in-tree",
                                     "error": "ran past the step limit of %g s; nothing more is started" % opt.step_timeout}))
            print(lines[-1], flush=True)
            return False
        final = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode != 0 or not final:
            lines.append(json.dumps({"point": point, "library": lib or "in-tree",
                                     "error": "exit status %d; nothing more is started" % done.returncode,
                                     "output": done.stdout[-400:]}))
            print(lines[-1], flush=True)
            return False
        lines.append(final[-1])
        print(final[-1], flush=True)
        return True

    ok = True
    for point in [t.strip() for t in opt.points.split(",") if t.strip()]:
        for lib in [None] + opt.variant:
            ok = ok and step(point, lib)
            if not ok:
                break
        if not ok:
            break
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("# tools/align_bench.py --points %s --iters %d --radius %g --reps %d --warmup %d --ref-scans %d%s\n"
                    % (opt.points, opt.iters, opt.radius, opt.reps, opt.warmup, opt.ref_scans,
                       "".join(" --variant " + v for v in opt.variant)))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
