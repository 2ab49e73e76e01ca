"""Time the incremental update of a landmark map (sgpr_landmark_update) against rebuilding the map
(sgpr_landmark_map) on synth.landmark_world.

    python tools/update_bench.py [--points 3x100,2x4541] [--reps N] [--warmup W] [--ref-scans Q] [--step-timeout S]
                                 [--world-cache DIR] [--out profiles/update.txt]

A point DxS is landmark_world with D drives of S scans.  The landmark map is built on the device from every drive but
the last at the true poses; the scans of the last drive (1xS-sized) are aligned to it from their true poses displaced by
N(0, 0.02) rad and N(0, 0.3) m (gates 2.0 then 0.75 m, landmarks with three or more observations), associated with all
landmarks (iters = 0) and folded in.  Every point runs in a process of its own under --step-timeout seconds; a point
that fails or runs out of time ends the run (nothing more is started on the device).  Per point, one JSON line: the
median of --reps update calls with events around the call, the inputs resident and the workspace allocated; the same for
sgpr_landmark_map rebuilding the whole map of D drives on the same poses - the yardstick: what a user without the update
has to run; the landmarks before and after, observed and new nodes, the share of updated landmarks whose count is the
batch map's; and whether the update of the first --ref-scans scans alone equals tests/landmark_update_ref.py bit for
bit.  No time is promised and none is asserted: the file records what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def timed(call, reps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def run_point(opt):
    import numpy as np
    import torch
    import landmark_update_ref as ref
    from sg_pr_amd import landmarks, synth
    D, S = (int(t) for t in opt.point.split("x"))
    if D < 2:
        raise SystemExit("a point needs a map and a drive to fold in: D >= 2")
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
    L = int(lm["num_landmarks"])
    rng = np.random.default_rng(500)
    truth = w["truth"][M:]
    start = synth._se2_compose(truth, synth._se2(rng.normal(0, 0.02, S), rng.normal(0, 0.3, S), rng.normal(0, 0.3, S)))
    cen, lab = torch.from_numpy(w["centers"][M:]).cuda(), torch.from_numpy(w["labels"][M:]).cuda()
    X = torch.from_numpy(start).cuda()
    use = landmarks.select(lm, min_count=3)
    for r in (2.0, 0.75):
        X = landmarks.align_async(cen, lab, X, lm, use=use, radius=r, iters=10)["poses"]
    assoc = landmarks.align_async(cen, lab, X, lm, iters=0)["node_landmark"]
    kw = dict(session_base=D - 1, node_base=M * N)
    ws = torch.empty(max(landmarks.update_workspace_bytes(S, N, L), 1), dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    up = landmarks.update(cen, lab, X, assoc, lm, workspace=ws, **kw)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    cap = up["num_landmarks"]
    update_ms = timed(lambda: landmarks.update_async(cen, lab, X, assoc, lm, workspace=ws, max_landmarks=cap, **kw), opt.reps,
                      opt.warmup)
    all_c, all_l = torch.from_numpy(w["centers"]).cuda(), torch.from_numpy(w["labels"]).cuda()
    all_x = torch.cat((torch.from_numpy(w["truth"][:M]).cuda(), X))
    ws_all = torch.empty(max(landmarks.workspace_bytes(D * S, N), 1), dtype=torch.uint8, device="cuda")
    batch = landmarks.build(all_c, all_l, all_x, starts=w["starts"], workspace=ws_all)
    bcap = batch["num_landmarks"]
    rebuild_ms = timed(lambda: landmarks.build_async(all_c, all_l, all_x, starts=w["starts"], workspace=ws_all, max_landmarks=bcap),
                       opt.reps, opt.warmup)
    holder = batch["node_landmark"].reshape(-1)[up["first"].long()]
    same = (batch["count"][holder.long()] == up["count"]).float().mean().item()
    rec = {"point": opt.point, "map_scans": M, "new_scans": S, "slots": N, "landmarks_before": L, "landmarks_after": cap,
           "observed": up["observed"], "new_nodes": up["new_nodes"], "live_nodes": up["live_nodes"],
           "workspace_MiB": ws.numel() / 2.0 ** 20, "first_call_ms": first_ms, "update_ms": update_ms,
           "rebuild_scans": D * S, "rebuild_landmarks": bcap, "rebuild_workspace_MiB": ws_all.numel() / 2.0 ** 20,
           "rebuild_ms": rebuild_ms, "rebuild_over_update": rebuild_ms / update_ms, "same_count_as_batch": same}
    q = min(opt.ref_scans, S)
    host_lm = {k: lm[k].cpu().numpy() for k in ref.RECORD}
    host_lm["sessions"] = host_lm["sessions"].view(np.uint64)
    part = landmarks.update(cen[:q], lab[:q], X[:q], assoc[:q], lm, **kw)
    t0 = time.perf_counter()
    want = ref.update(w["centers"][M:M + q], w["labels"][M:M + q], X[:q].cpu().numpy(), assoc[:q].cpu().numpy(), host_lm, **kw)
    rec["ref_scans"], rec["ref_s"] = q, time.perf_counter() - t0
    rec["equal_to_reference"] = bool(all(part[k].cpu().numpy().tobytes() == want[k].tobytes() for k in ref.RECORD + ("node_landmark",))
                                     and [part[k] for k in ("num_landmarks", "live_nodes", "observed", "new_nodes")] == want["num"].tolist())
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default="3x100,2x4541")
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-scans", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--world-cache", default=None)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    if opt.point is not None:
        return run_point(opt)
    lines = ["# tools/update_bench.py " + " ".join(sys.argv[1:])]
    for point in opt.points.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup", str(opt.warmup),
               "--ref-scans", str(opt.ref_scans)] + (["--world-cache", opt.world_cache] if opt.world_cache else [])
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=opt.step_timeout)
        except subprocess.TimeoutExpired:
            print("point %s ran out of time: stopping" % point, flush=True)
            break
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            print("point %s failed with status %d: stopping" % (point, done.returncode), flush=True)
            break
        lines += [t for t in done.stdout.splitlines() if t.startswith("{")]
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(lines) == 1 + len(opt.points.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
