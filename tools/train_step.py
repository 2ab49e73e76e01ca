"""Time one training step at the reference's batch (128 pairs = 256 graphs, N = 100, K = 10): the fused HIP EdgeConv
path (sg_pr_amd.train) vs the dense formulation of tests/train_ref.py in fp32 on the same GPU.  Prints one JSON line
(median ms per step, peak activation MB); run it under `rocprofv3 --kernel-trace --stats -- python tools/train_step.py
--fused-only` for the per-kernel breakdown.

--in-batch: instead, in one call and alternating step by step, the classic step (`fused_ms`, the listed pairs), the
in-batch step on the HIP all-pairs tail (train_loss_in_batch) and the in-batch step with the tail in torch ops (gather
the labelled pairs to [P, F], train.tensor_network, train.head, weighted BCE); the classes come from the poses of a
synth.world_sequence with as many scans as the batch has graphs.  Median, 10th / 90th percentile ms and peak
activation MB of each.  `--in-batch --only hip` runs the HIP in-batch step alone (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--in-batch", action="store_true")
    ap.add_argument("--only", choices=("classic", "hip", "torch"), default=None)
    a = ap.parse_args()
    from oracle import sgpr_oracle
    from sg_pr_amd import synth
    from sg_pr_amd.sg_net import SG
    from sg_pr_amd.parser_sg import sgpr_args
    from sg_pr_amd.train import dense_features, train_loss
    import train_ref

    c, l, _ = synth.make_graphs(2 * a.pairs, 100, 20, 90, 0, kitti_like=True)
    feats = dense_features(torch.from_numpy(c).cuda(), torch.from_numpy(l).cuda())
    target = (torch.arange(a.pairs, device="cuda") % 2).float()
    model = SG(sgpr_args(), 12)
    model.load_state_dict(sgpr_oracle.load_checkpoint(os.path.join(REPO, "tests", "golden", "model.pth")))
    model = model.cuda().train()
    _, _, lists = train_loss(model, feats, target, updates=0)
    params = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}

    def fused():
        model.zero_grad(set_to_none=True)
        loss, _, _ = train_loss(model, feats, target, updates=0)
        loss.backward()

    def dense():
        for v in params.values():
            v.grad = None
        loss, _, _ = train_ref.train_step_loss(params, feats, target, lists)
        loss.backward()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    out = {"pairs": a.pairs, "graphs": 2 * a.pairs, "N": 100, "K": 10, "steps": a.steps}
    if a.in_batch:
        return in_batch(a, out, model, feats, fused)
    out["fused_ms"], out["fused_peak_mb"] = timed(fused)
    if not a.fused_only:
        out["dense_fp32_ms"], out["dense_fp32_peak_mb"] = timed(dense)
        out["speedup"] = out["dense_fp32_ms"] / out["fused_ms"]
        out["memory_ratio"] = out["dense_fp32_peak_mb"] / out["fused_peak_mb"]
    print(json.dumps(out))


def in_batch(a, out, model, feats, classic):
    import numpy as np
    import train_pairs_ref
    from sg_pr_amd import synth
    from sg_pr_amd.train import attention, embed_train, pair_classes, train_loss_in_batch

    g = 2 * a.pairs
    _, _, _, poses = synth.world_sequence(num_graphs=g, node_num=100, seed=5)
    cls_np = pair_classes(poses[:, [3, 11]], np.arange(g))
    cls = torch.from_numpy(cls_np).cuda()
    out.update(pairs_in_loss=int((cls_np <= 1).sum()), positives=int((cls_np == 1).sum()),
               negatives=int((cls_np == 0).sum()))

    def hip():
        model.zero_grad(set_to_none=True)
        loss, _, _ = train_loss_in_batch(model, feats, cls, 1.0, 1.0, updates=0)
        loss.backward()

    def torch_tail():
        model.zero_grad(set_to_none=True)
        emb, _ = embed_train(model, feats, 0)
        rep, _ = attention(model.attention, emb)
        loss, _, _ = train_pairs_ref.gathered_pairs_loss(rep[:, :, 0], cls, model)
        loss.backward()

    fns = {"classic": classic, "hip": hip, "torch": torch_tail}
    if a.only:
        fns = {a.only: fns[a.only]}
    ts = {k: [] for k in fns}
    peak = {}
    for k, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(a.steps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    names = {"classic": "fused", "hip": "in_batch_hip", "torch": "in_batch_torch_tail"}
    for k, v in ts.items():
        v.sort()
        n = names[k]
        out[n + "_ms"], out[n + "_p10_ms"], out[n + "_p90_ms"] = v[len(v) // 2], v[len(v) // 10], v[(9 * len(v)) // 10]
        out[n + "_peak_mb"] = peak[k]
    if "fused_ms" in out and "in_batch_hip_ms" in out:
        out["in_batch_hip_over_classic"] = out["in_batch_hip_ms"] / out["fused_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
