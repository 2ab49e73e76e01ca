"""Time one training step at the reference's batch (128 pairs = 256 graphs, N = 100, K = 10): the fused HIP EdgeConv
path (sg_pr_amd.train) vs the dense formulation of tests/train_ref.py in fp32 on the same GPU.  Prints one JSON line
(median ms per step, peak activation MB); run it under `rocprofv3 --kernel-trace --stats -- python tools/train_step.py
--fused-only` for the per-kernel breakdown."""
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
    out["fused_ms"], out["fused_peak_mb"] = timed(fused)
    if not a.fused_only:
        out["dense_fp32_ms"], out["dense_fp32_peak_mb"] = timed(dense)
        out["speedup"] = out["dense_fp32_ms"] / out["fused_ms"]
        out["memory_ratio"] = out["dense_fp32_peak_mb"] / out["fused_peak_mb"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
