"""Time the landmark map (sgpr_landmark_map) on synth.landmark_world beside a host partition.

    python tools/landmark_bench.py [--points 1x600,1x4541,5x4541] [--reps N] [--warmup W] [--ref-links L]
                                   [--step-timeout S] [--out profiles/landmarks.txt]

A point DxS is landmark_world with D drives of S scans at its true poses.  Every point runs in a process of its own under
--step-timeout seconds; a point that fails or runs out of time ends the run (nothing more is started on the device).  Per
point, one JSON line: the median wall time of the call (events around it) with the inputs already on the device and the
workspace allocated, nodes and landmarks, and the figures of metrics.map_sharpness.  The host column is the same
partition by scipy.spatial.cKDTree.query_pairs + scipy.sparse.csgraph.connected_components per label, when scipy imports
and the pairs within the radius (counted first) number at most --ref-links; beyond that, or without scipy, the line says
"not measured".  Where the NumPy reference (tests/landmark_ref.py) can reach - its links at most --ref-links as well -
every output is compared with it bit for bit; elsewhere the line says that it was not.  No speed is gated on: the file
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


def host_partition(m, lab, live, radius, tau_z, limit):
    """connected components by scipy -> (component of every live node as its lowest member, seconds, pairs) or a reason"""
    import numpy as np
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
    except ImportError:
        return "not measured: scipy does not import"
    t0 = time.perf_counter()
    nodes = np.flatnonzero(live)
    trees = {int(l): (nodes[lab[nodes] == l], cKDTree(m[nodes[lab[nodes] == l], :2])) for l in np.unique(lab[nodes])}
    pairs = sum((int(t.count_neighbors(t, radius)) - idx.size) // 2 for idx, t in trees.values())
    if pairs > limit:
        return "not measured: %d pairs within the radius exceed --ref-links %d" % (pairs, limit)
    a, b = [], []
    for idx, tree in trees.values():
        p = tree.query_pairs(radius, output_type="ndarray")
        p = p[np.abs(m[idx[p[:, 0]], 2] - m[idx[p[:, 1]], 2]) <= tau_z]
        a.append(idx[p[:, 0]])
        b.append(idx[p[:, 1]])
    a, b = np.concatenate(a), np.concatenate(b)
    P = m.shape[0]
    _, comp = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(P, P)), directed=False)
    low = np.full(comp.max() + 1, P, np.int64)
    np.minimum.at(low, comp[nodes], nodes)
    return low[comp[nodes]], time.perf_counter() - t0, pairs


def run_point(opt):
    import numpy as np
    import torch
    import landmark_ref as ref
    from sg_pr_amd import landmarks, metrics, synth
    D, S = (int(t) for t in opt.point.split("x"))
    w = synth.landmark_world(0, scans=S, sessions=D, closures=0)
    G, N = w["labels"].shape
    dev = {name: torch.from_numpy(w[name]).cuda() for name in ("centers", "labels", "truth")}
    ws = torch.empty(landmarks.workspace_bytes(G, N), dtype=torch.uint8, device="cuda")

    def call():
        return landmarks.build_async(dev["centers"], dev["labels"], dev["truth"], starts=w["starts"], workspace=ws)

    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    rec = {"point": opt.point, "scans": G, "slots": N, "workspace_MiB": ws.numel() / 2.0 ** 20,
           "first_call_ms": 1e3 * (time.perf_counter() - t0)}
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
    found, live_n = (int(v) for v in out["num"].tolist())
    got = {k: v.cpu().numpy() for k, v in out.items()}
    lm = {k: got[k][:found] for k in ("count", "spread", "sessions")}
    rec.update({"call_ms": float(np.median(times)), "cell_layout": "linked list per cell", "live_nodes": live_n,
                "landmarks_found": found, "nodes_per_s": live_n / (1e-3 * float(np.median(times)))})
    rec.update(metrics.map_sharpness(lm))
    print(json.dumps({"point": opt.point, "progress": "device timed", "call_ms": rec["call_ms"]}), flush=True)
    m = ref.map_points(w["centers"], w["truth"]).reshape(-1, 3)
    lab = w["labels"].reshape(-1)
    live = got["node_landmark"].reshape(-1) >= 0
    host = host_partition(m, lab, live, 0.75, 0.75, opt.ref_links)
    if isinstance(host, str):
        rec["host_scipy"] = host
    else:
        roots, took, pairs = host
        first = got["first"][:found][got["node_landmark"].reshape(-1)[live]]
        rec.update({"host_scipy_s": took, "host_scipy_pairs": pairs, "partition_equal_to_scipy": bool((first == roots).all())})
    if isinstance(host, str) and "exceed" in host:
        rec["equal_to_reference"] = "not checked: beyond the reference's reach (--ref-links)"
    else:
        t0 = time.perf_counter()
        want = ref.landmark_map(w["centers"], w["labels"], w["truth"], starts=w["starts"])
        rec["ref_s"] = time.perf_counter() - t0
        rec["ref_links"] = want["links"]
        rec["equal_to_reference"] = bool(
            got["num"].tolist() == want["num"].tolist() and got["node_landmark"].tobytes() == want["node_landmark"].tobytes() and
            all(got[k][:found].tobytes() == want[k].tobytes() for k in ("center", "label", "count", "first", "sessions", "spread")))
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x600,1x4541,5x4541")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-links", type=int, default=60000000, help="links the host partitions are asked to form at most")
    ap.add_argument("--step-timeout", type=float, default=400.0, help="seconds per point")
    ap.add_argument("--out", default=None)
    ap.add_argument("--point", default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args(argv)
    if opt.point is not None:
        return run_point(opt)
    lines = []
    for point in [t.strip() for t in opt.points.split(",") if t.strip()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(opt.reps), "--warmup",
               str(opt.warmup), "--ref-links", str(opt.ref_links)]
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
            f.write("# tools/landmark_bench.py --points %s --reps %d --warmup %d --ref-links %d\n"
                    % (opt.points, opt.reps, opt.warmup, opt.ref_links))
            f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
