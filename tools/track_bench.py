"""Time the tracking of drives through a landmark map (sgpr_landmark_track) on synth.landmark_world,
against what the library offered before it for the same result: a Python loop over the scans with one
landmarks.align_async call per gate and one read per scan.

    python tools/track_bench.py [--points 1x300,1x4541,16x300] [--reps 15] [--warmup 3] [--loop-reps N] [--ref-scans Q]
                                [--step-timeout S] [--out profiles/track.txt]

A point TxS is landmark_world(0, scans=S) with three drives: the landmark map is built on the device from drives 0 and 1
at the true poses, its landmarks with three or more observations are in use, and drive 2 is tracked from its odometry
and its true first pose displaced by N(0, 0.02) rad and N(0, 0.3) m - T times over, as T tracks of one call with T
different displacements.  Gates 2.0 and 0.75 m, an 8.0 m gate after a lost scan, 10 iterations, min_matched 10.
Every point runs in a process of its own under --step-timeout seconds; a point that fails or runs out of time ends the
run (nothing more is started on the device).  Per point, one JSON line: the median of --reps calls after --warmup calls,
events around the call, the inputs resident and the workspace allocated; the same for the loop - per scan index the
predictions of the T tracks composed on the host, one align_async of those T scans per gate, one read of the poses and
of every gate's counts - with host clocks around it; whether every output of the two is the same bytes;
tests/landmark_track_ref.py on the first --ref-scans scans of the first track and whether the call equals it there.
No time is promised and none is asserted: the file records what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

RADII, REACQUIRE, ITERS, MIN_NODES, MIN_MATCHED = (2.0, 0.75), (8.0,), 10, 6, 10


def run_point(opt):
    import numpy as np
    import torch
    import landmark_track_ref as ref
    from sg_pr_amd import landmarks, synth
    T, S = (int(t) for t in opt.point.split("x"))
    w = synth.landmark_world(0, scans=S, closures=0)
    M = 2 * S
    lm = landmarks.build(w["centers"][:M], w["labels"][:M], w["truth"][:M], starts=w["starts"][:2])
    use = landmarks.select(lm, min_count=3)
    rng = np.random.default_rng(900)
    truth = np.tile(w["truth"][M:], (T, 1))
    init = synth._se2_compose(np.tile(w["truth"][M], (T, 1)),
                              synth._se2(rng.normal(0, 0.02, T), rng.normal(0, 0.3, T), rng.normal(0, 0.3, T)))
    host = {"centers": np.tile(w["centers"][M:], (T, 1, 1)), "labels": np.tile(w["labels"][M:], (T, 1)),
            "odom": np.tile(w["odom"][M:], (T, 1))}
    starts = np.arange(T, dtype=np.int32) * S
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    dev_init = torch.from_numpy(init).cuda()
    Q, N = host["labels"].shape
    L = int(lm["num_landmarks"])
    n_stages = len(RADII) + len(REACQUIRE)
    ws = torch.empty(max(landmarks.track_workspace_bytes(Q, N, L, n_stages), 1), dtype=torch.uint8, device="cuda")

    def call():
        return landmarks.track_async(dev["centers"], dev["labels"], dev["odom"], dev_init, lm, use=use, starts=starts, radii=RADII,
                                     reacquire_radii=REACQUIRE, iters=ITERS, min_nodes=MIN_NODES, min_matched=MIN_MATCHED,
                                     workspace=ws)

    # the loop: what the library offered before this call
    cen3, lab2 = dev["centers"].reshape(T, S, N, 3), dev["labels"].reshape(T, S, N)
    aws = torch.empty(max(landmarks.align_workspace_bytes(T, N, L), 1), dtype=torch.uint8, device="cuda")
    stages = [(r, True) for r in REACQUIRE] + [(r, False) for r in RADII]
    odom3 = host["odom"].reshape(T, S, 4)

    def loop():
        out = {"poses": torch.empty(T, S, 4, dtype=torch.float64, device="cuda"), "pred": np.zeros((T, S, 4)),
               "node_landmark": torch.empty(T, S, N, dtype=torch.int32, device="cuda"), "stat": np.zeros((T, S, 4), np.int32),
               "rms": torch.empty(T, S, dtype=torch.float64, device="cuda")}
        A, lost = init.copy(), np.zeros(T, bool)
        delta = synth._se2_compose(synth._se2_inverse(odom3[:, :-1]), odom3[:, 1:])       # (the header's formulas, on arrays)
        for i in range(S):
            P = A if i == 0 else synth._se2_compose(A, delta[:, i - 1])
            c, l = cen3[:, i].contiguous(), lab2[:, i].contiguous()
            X = torch.from_numpy(P).cuda()
            run = []
            for r, wide in stages:
                if wide and not lost.any():
                    continue
                res = landmarks.align_async(c, l, X, lm, use=use, radius=r, iters=ITERS, min_nodes=MIN_NODES, workspace=aws)
                if wide:                                        # the tracks that were not lost skip the wide gate
                    X = torch.where(torch.from_numpy(lost).cuda()[:, None], res["poses"], X)
                else:
                    X, last = res["poses"], res
                run.append((res["stat"], wide))
            back = torch.cat([X.reshape(-1)] + [st.to(torch.float64).reshape(-1) for st, _ in run]).cpu().numpy()  # the one read
            X_h = back[:4 * T].reshape(T, 4)
            steps, flags = np.zeros(T, np.int64), np.where(lost, ref.REACQUIRE, 0)
            for j, (_, wide) in enumerate(run):
                stat = back[4 * T * (j + 1):4 * T * (j + 2)].reshape(T, 4).astype(np.int64)
                took = lost if wide else np.ones(T, bool)
                steps += np.where(took, stat[:, 2], 0)
                flags |= np.where(took, stat[:, 3], 0)
            lost = stat[:, 0] < MIN_MATCHED
            A = np.where(lost[:, None], P, X_h)
            out["poses"][:, i] = torch.from_numpy(A).cuda()
            out["pred"][:, i] = P
            out["node_landmark"][:, i] = last["node_landmark"]
            out["rms"][:, i] = last["rms"]
            out["stat"][:, i, :2] = stat[:, :2]
            out["stat"][:, i, 2] = steps
            out["stat"][:, i, 3] = flags | np.where(lost, ref.LOST, 0)
        torch.cuda.synchronize()
        return out

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
    loop_times, mine = [], None
    for j in range(opt.loop_warmup + opt.loop_reps):
        t0 = time.perf_counter()
        mine = loop()
        if j >= opt.loop_warmup:
            loop_times.append(1000.0 * (time.perf_counter() - t0))

    def err(X):
        return np.hypot(X[:, 2] - truth[:, 2], X[:, 3] - truth[:, 3])
    rec = {"point": opt.point, "tracks": T, "scans_per_track": S, "slots": N, "landmarks": L, "in_use": int(use.sum()),
           "radii": list(RADII), "reacquire_radii": list(REACQUIRE), "iters": ITERS, "min_matched": MIN_MATCHED,
           "call_ms": float(np.median(times)), "calls_ms": [round(t, 3) for t in times], "call_us_per_scan": 1000.0 * float(np.median(times)) / Q,
           "workspace_KiB": ws.numel() / 1024.0, "num": got["num"].tolist(), "median_error_m": float(np.median(err(got["poses"]))),
           "max_error_m": float(err(got["poses"]).max())}
    if mine is not None:
        same = {"poses": mine["poses"].cpu().numpy().reshape(Q, 4).tobytes() == got["poses"].tobytes(),
                "pred": mine["pred"].reshape(Q, 4).tobytes() == got["pred"].tobytes(),
                "node_landmark": mine["node_landmark"].cpu().numpy().reshape(Q, N).tobytes() == got["node_landmark"].tobytes(),
                "rms": mine["rms"].cpu().numpy().reshape(Q).tobytes() == got["rms"].tobytes(),
                "stat": mine["stat"].reshape(Q, 4).tobytes() == got["stat"].tobytes()}
        rec.update({"loop_ms": float(np.median(loop_times)), "loops_ms": [round(t, 1) for t in loop_times],
                    "loop_us_per_scan": 1000.0 * float(np.median(loop_times)) / Q, "loop_equal_bytes": same,
                    "loop_over_call": float(np.median(loop_times) / np.median(times))})
    if opt.ref_scans > 0:
        n = min(S, opt.ref_scans)
        t0 = time.perf_counter()
        want = ref.track(host["centers"][:n], host["labels"][:n], host["odom"][:n], init[:1], lm["center"].cpu().numpy(),
                         lm["label"].cpu().numpy(), use.cpu().numpy(), radii=REACQUIRE + RADII, n_reacquire=len(REACQUIRE), iters=ITERS,
                         min_nodes=MIN_NODES, min_matched=MIN_MATCHED)
        rec["ref_scans"] = n
        rec["ref_s"] = time.perf_counter() - t0
        rec["equal_to_reference"] = bool(all(got[k][:n].tobytes() == want[k].tobytes() for k in ("poses", "pred", "node_landmark", "stat", "rms")))
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x300,1x4541,16x300")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=None, help="timed runs of the Python loop (default: --reps)")
    ap.add_argument("--loop-warmup", type=int, default=None, help="untimed runs of the Python loop before them (default: --warmup)")
    ap.add_argument("--ref-scans", type=int, default=100, help="scans of the first track the NumPy reference is run and compared on")
    ap.add_argument("--step-timeout", type=float, default=420.0, help="seconds per point")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    opt.loop_reps = opt.reps if opt.loop_reps is None else opt.loop_reps
    opt.loop_warmup = opt.warmup if opt.loop_warmup is None else opt.loop_warmup
    if opt.point is not None:
        return run_point(opt)
    lines = []
    for point in [t.strip() for t in opt.points.split(",") if t.strip()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup", str(opt.warmup),
               "--loop-reps", str(opt.loop_reps), "--loop-warmup", str(opt.loop_warmup), "--ref-scans", str(opt.ref_scans)]
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
            f.write("# tools/track_bench.py --points %s --reps %d --warmup %d --loop-reps %d --loop-warmup %d --ref-scans %d\n"
                    % (opt.points, opt.reps, opt.warmup, opt.loop_reps, opt.loop_warmup, opt.ref_scans))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
