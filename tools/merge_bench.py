"""Time the record-level merge of two landmark maps (sgpr_landmark_merge) against rebuilding the map of
both drives from their scans (sgpr_landmark_map) on synth.landmark_world.

    python tools/merge_bench.py [--points 100,4541] [--reps N] [--warmup W] [--step-timeout S] [--world-cache DIR]
                                [--out profiles/merge.txt]

A point S is landmark_world(0, scans=S): the landmark maps of drive 0 and of drive 1 are built apart on the device at
the true poses and merged (session_shift 1, first_base = the nodes of drive 0).  Every point runs in a process of its own
under --step-timeout seconds; a point that fails or runs out of time ends the run (nothing more is started on the device).
Per point, one JSON line: the median of --reps merge calls after --warmup more, with events around the call, the inputs
resident and the workspace allocated; the same for sgpr_landmark_map rebuilding the map from the scans of both drives -
the yardstick: what a user without the merge has to run; the same for the compaction of the merged map under a mask that
drops the landmarks seen once; the landmarks of the two maps, of the merged map and of the batch map, the share of merged
landmarks whose count is the batch map's; and whether the merge equals tests/landmark_merge_ref.py bit for bit.  No time
is promised and none is asserted: the file records what was measured."""
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


def world(S, cache):
    import numpy as np
    from sg_pr_amd import synth
    cached = os.path.join(cache, "landmark_world_0_%d.npz" % S) if cache else None
    if cached and os.path.exists(cached):
        return dict(np.load(cached))
    w = synth.landmark_world(0, scans=S)
    w = {k: w[k] for k in ("centers", "labels", "truth")}
    if cached:
        os.makedirs(cache, exist_ok=True)
        np.savez(cached, **w)
    return w


def run_point(opt):
    import numpy as np
    import torch
    import landmark_merge_ref as ref
    from sg_pr_amd import landmarks
    S = int(opt.point)
    w = world(S, opt.world_cache)
    N = w["labels"].shape[1]
    cen, lab, X = (torch.from_numpy(np.ascontiguousarray(w[k][:2 * S])).cuda() for k in ("centers", "labels", "truth"))
    A = landmarks.build(cen[:S], lab[:S], X[:S])
    B = landmarks.build(cen[S:], lab[S:], X[S:])
    La, Lb = int(A["num_landmarks"]), int(B["num_landmarks"])
    kw = dict(session_shift=1, first_base=S * N)
    ws = torch.empty(max(landmarks.merge_workspace_bytes(La, Lb), 1), dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    mg = landmarks.merge(A, B, workspace=ws, **kw)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    cap = mg["num_landmarks"]
    merge_ms = timed(lambda: landmarks.merge_async(A, B, workspace=ws, max_landmarks=cap, **kw), opt.reps, opt.warmup)
    keep = mg["count"] >= 2
    small = landmarks.compact(mg, keep=keep)
    ws_c = torch.empty(max(landmarks.merge_workspace_bytes(cap, 0), 1), dtype=torch.uint8, device="cuda")
    mask = keep.to(torch.uint8)
    compact_ms = timed(lambda: landmarks.merge_async(mg, keep_a=mask, workspace=ws_c, max_landmarks=small["num_landmarks"]),
                       opt.reps, opt.warmup)
    ws_all = torch.empty(max(landmarks.workspace_bytes(2 * S, N), 1), dtype=torch.uint8, device="cuda")
    batch = landmarks.build(cen, lab, X, starts=[0, S], workspace=ws_all)
    bcap = batch["num_landmarks"]
    rebuild_ms = timed(lambda: landmarks.build_async(cen, lab, X, starts=[0, S], workspace=ws_all, max_landmarks=bcap), opt.reps,
                       opt.warmup)
    holder = batch["node_landmark"].reshape(-1)[mg["first"].long()]
    same = (batch["count"][holder.long()] == mg["count"]).float().mean().item()
    rec = {"scans_per_drive": S, "slots": N, "landmarks_a": La, "landmarks_b": Lb, "merged": cap, "fused": mg["fused"],
           "batch_landmarks": bcap, "same_count_as_batch": same, "workspace_MiB": ws.numel() / 2.0 ** 20, "first_call_ms": first_ms,
           "merge_ms": merge_ms, "compact_kept": small["num_landmarks"], "compact_ms": compact_ms, "rebuild_scans": 2 * S,
           "rebuild_workspace_MiB": ws_all.numel() / 2.0 ** 20, "rebuild_ms": rebuild_ms, "rebuild_over_merge": rebuild_ms / merge_ms}
    host = []
    for lm in (A, B):
        h = {k: lm[k].cpu().numpy() for k in ref.RECORD}
        h["sessions"] = h["sessions"].view(np.uint64)
        host.append(h)
    t0 = time.perf_counter()
    want = ref.merge(*host, **kw)
    rec["ref_s"] = time.perf_counter() - t0
    rec["equal_to_reference"] = bool(all(mg[k].cpu().numpy().tobytes() == want[k].tobytes() for k in ref.RECORD + ("old_to_new",))
                                     and [mg["num_landmarks"], *mg["dropped"], mg["fused"]] == want["num"].tolist())
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default="100,4541")
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--world-cache", default=None)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    if opt.point is not None:
        return run_point(opt)
    lines = ["# tools/merge_bench.py " + " ".join(sys.argv[1:])]
    for point in opt.points.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup", str(opt.warmup)] + \
              (["--world-cache", opt.world_cache] if opt.world_cache else [])
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
