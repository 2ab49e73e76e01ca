"""Float64 reference of the per-graph half and the tail for ANY architecture, with the library's stated neighbour rule.
TEST INFRASTRUCTURE ONLY (like oracle/sgpr_oracle.py, whose dtype-generic pieces it reuses on float64 state dicts).

What it restates itself is dgcnn.knn: the oracle's torch.topk leaves the order among equal keys unspecified, so a graph
with fewer than K padding slots (one-hot rows tie EXACTLY across labels) has no defined neighbour sets there.  Here the
candidates of row i are ordered by true squared distance (a sum of squared differences in float64, never the expansion),
then by index ascending (a stable sort); the first K are taken, self included - the rule sgpr_wide.hip, sgpr_generic.hip
and sgpr_knn document.

Every EdgeConv layer and row also gets a MARGIN that tells a wrong neighbour from a legitimate fp32 near-tie without a
debug dump: the first candidate NOT taken whose feature row is not a copy of a taken row (swapping copies changes
nothing), its distance minus the K-th taken distance, over S = |x_i|^2 + max_j |x_j|^2.
inf = nothing left to confuse (K = N, or only copies of taken rows remain).  0 is legal in the first semantic layer only:
one-hot rows give exact keys in every arithmetic (fp32 FMA chains and f16 planes included), so the index rule decides
those ties identically here and in the kernels.  A graph is SETTLED at tau when every margin outside sem1 is >= tau (and
every sem1 margin is 0 or >= tau).

tau is measured, not chosen (python tests/any_shape_ref.py, on a CPU; it walks every row of the sweep table):
  e32      = max |pd32 - pd64| / S of the oracle's own fp32 neg_sq_dist on the reference's layer inputs rounded to fp32
  TAU_PLAIN = 16 e32   (another summation order of equal quality may move either key of a pair by that much)
  TAU_WIDE  = 4 TAU_PLAIN   (two f16 planes carry 22 bits, not 24)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle import sgpr_oracle as oracle   # noqa: E402

LAYERS = ("xyz1", "xyz2", "xyz3", "sem1", "sem2", "sem3")
_PREFIX = {"xyz1": "dgcnn_s_conv1", "xyz2": "dgcnn_s_conv2", "xyz3": "dgcnn_s_conv3",
           "sem1": "dgcnn_f_conv1", "sem2": "dgcnn_f_conv2", "sem3": "dgcnn_f_conv3"}

# Measured by `python tests/any_shape_ref.py` over all embed rows of tests/test_gpu_any_shape_sweep.py::EMBED_ROWS
# (worst row: see DESIGN.md, "Any-shape routes as tested"):
E32 = 9.14e-7
TAU_PLAIN = 16 * E32
TAU_WIDE = 4 * TAU_PLAIN


def state_dict_f64(sd):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}


COPY_EPS = 1e-12       # rows closer than this (relative to the layer's largest value) are copies of each other
TIE_EPS = 1e-12        # a gap at the cut below this (relative to S) is a tie: walk past the copies of taken rows


def sq_dist(x):
    """x [C,N] float64 -> ([N,N] true squared distances, [N,N] largest coordinate difference), channel by channel"""
    n = x.shape[1]
    d = torch.zeros(n, n, dtype=torch.float64)
    far = torch.zeros(n, n, dtype=torch.float64)
    for c in range(x.shape[0]):
        diff = x[c].unsqueeze(1) - x[c].unsqueeze(0)
        d.addcmul_(diff, diff)
        torch.maximum(far, diff.abs_(), out=far)
    return d, far


def copies(x):
    """bool [N,N]: rows i and j of x [C,N] are copies - equal in exact arithmetic (padding slots, nodes of one label with
    the same neighbourhood).  A float64 GEMM may round the columns of its edge blocks differently from the others, so
    copies are equal to ~1e-15 and not always to the bit: the test is COPY_EPS, far below anything a gate could see."""
    return sq_dist(x)[1] <= COPY_EPS * max(1.0, float(x.abs().max()))


def select(x, k):
    """x [C,N] float64 -> (idx int64 [N,k] in (distance, index) order, margin float64 [N])."""
    n = x.shape[1]
    d, far = sq_dist(x)
    ds, order = torch.sort(d, dim=1, stable=True)
    idx = order[:, :k].contiguous()
    margin = torch.full((n,), float("inf"), dtype=torch.float64)
    if k == n:
        return idx, margin
    xx = (x * x).sum(0)
    s = xx + xx.max()
    dk = ds[:, k - 1]
    gap = ds[:, k] - dk
    tied = gap <= TIE_EPS * s
    margin = torch.where(tied, margin, gap / s)
    if tied.any():
        # the first candidate left out that is not a copy of a taken row (a copy of one is as far as it is: at the cut)
        same = (far <= COPY_EPS * max(1.0, float(x.abs().max()))).numpy()
        dsn, on, sn = ds.numpy(), order.numpy(), s.numpy()
        for i in torch.nonzero(tied).reshape(-1).tolist():
            other = ~same[on[i, k:]][:, on[i, :k]].any(axis=1)
            if other.any():
                p = k + int(np.argmax(other))
                margin[i] = max(dsn[i, p] - dsn[i, k - 1], 0.0) / sn[i] if sn[i] > 0 else float("inf")
    return idx, margin


def _edgeconv(x, sd, prefix, k):
    """x [C,N] float64 -> (y [Cout,N], idx [N,k], margin [N]); sg_net.py:50-73 on the selected lists"""
    idx, margin = select(x, k)
    z = F.conv2d(oracle.graph_feature(x.unsqueeze(0), k, idx.unsqueeze(0)), sd[prefix + ".0.weight"])
    z = F.leaky_relu(oracle._bn(z, sd, prefix), oracle.LRELU_SLOPE)
    return z.max(dim=-1)[0][0], idx, margin


def embed(sd64, feats, k):
    """sd64: float64 state dict; feats [G,3+L,N] (any float dtype) -> dict of float64 tensors:
    layers {name: [G,Cout,N]}, inputs {name: [G,Cin,N]}, idx {name: [G,N,k]}, margins {name: [G,N]}, emb [G,N,F3],
    att [G,N], pooled [G,F3].  One graph at a time (the (1024, 64) case holds 270 MB per layer and graph)."""
    feats = feats.double()
    out = {"layers": {n: [] for n in LAYERS}, "inputs": {n: [] for n in LAYERS}, "idx": {n: [] for n in LAYERS},
           "margins": {n: [] for n in LAYERS}, "emb": [], "att": [], "pooled": []}
    with torch.no_grad():
        for g in range(feats.shape[0]):
            ends = []
            for branch, x in (("xyz", feats[g, :3]), ("sem", feats[g, 3:])):
                for l in (1, 2, 3):
                    name = "%s%d" % (branch, l)
                    out["inputs"][name].append(x)
                    x, idx, margin = _edgeconv(x, sd64, _PREFIX[name], k)
                    out["layers"][name].append(x)
                    out["idx"][name].append(idx)
                    out["margins"][name].append(margin)
                ends.append(x)
            z = F.conv1d(torch.cat(ends, dim=0).unsqueeze(0), sd64["dgcnn_conv_end.0.weight"])
            e = F.leaky_relu(oracle._bn(z, sd64, "dgcnn_conv_end"), oracle.LRELU_SLOPE).permute(0, 2, 1)
            p, a = oracle.attention(sd64, e)
            out["emb"].append(e[0])
            out["att"].append(a.reshape(-1))
            out["pooled"].append(p.reshape(-1))
    for key in ("layers", "inputs", "idx", "margins"):
        out[key] = {n: torch.stack(v) for n, v in out[key].items()}
    for key in ("emb", "att", "pooled"):
        out[key] = torch.stack(out[key])
    return out


def settled(ref, tau):
    """bool [G]: every margin outside sem1 >= tau, every sem1 margin 0 (exact one-hot ties: the index rule) or >= tau"""
    ok = torch.ones(ref["emb"].shape[0], dtype=torch.bool)
    for name in LAYERS:
        m = ref["margins"][name]
        good = (m >= tau) | ((m == 0) if name == "sem1" else torch.zeros_like(m, dtype=torch.bool))
        ok &= good.all(dim=1)
    return ok


def exact_ties_outside_sem1(ref):
    return sum(int((ref["margins"][n] == 0).sum()) for n in LAYERS if n != "sem1")


def tail(sd64, rows, cols, chunk=8):
    """float64 scores [R,M] of every (row, col) pair of pooled vectors: oracle.tensor_network + head in float64"""
    rows, cols = torch.as_tensor(rows).double(), torch.as_tensor(cols).double()
    r, m = rows.shape[0], cols.shape[0]
    out = torch.empty(r, m, dtype=torch.float64)
    with torch.no_grad():
        for i0 in range(0, r, chunk):
            part = rows[i0:i0 + chunk]
            a = part.repeat_interleave(m, dim=0).unsqueeze(-1)
            b = cols.repeat(part.shape[0], 1).unsqueeze(-1)
            out[i0:i0 + chunk] = oracle.head(sd64, oracle.tensor_network(sd64, a, b)).view(part.shape[0], m)
    return out


def key_error_fp32(ref):
    """e32 of one reference result: max over layers, graphs, rows of |pd32 - pd64| / S on the layer inputs rounded to fp32"""
    worst = 0.0
    for name in LAYERS:
        x32 = ref["inputs"][name].float()
        pd32 = oracle.neg_sq_dist(x32).double()
        x = x32.double()
        pd64 = oracle.neg_sq_dist(x)
        xx = (x * x).sum(1)                                            # [G,N]
        s = xx + xx.max(dim=1, keepdim=True)[0]
        live = s > 0                                                   # (an all-zero graph: every key is exactly 0)
        err = (pd32 - pd64).abs().amax(dim=2)
        if live.any():
            worst = max(worst, float((err[live] / s[live]).max()))
        assert float(err[~live].max() if (~live).any() else 0.0) == 0.0
    return worst


if __name__ == "__main__":
    # the measurement behind E32 / TAU_*: every embed row of the sweep, the graphs the GPU tests run
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_gpu_any_shape_sweep as sweep
    worst = (0.0, None)
    for row in sweep.EMBED_ROWS:
        case = sweep.host_case(row["id"])
        e = key_error_fp32(case["ref"])
        ok = settled(case["ref"], sweep.row_tau(row))
        worst_margin = torch.stack([case["ref"]["margins"][n].min(dim=1)[0] for n in LAYERS if n != "sem1"]).min(dim=0)[0]
        fills = (case["labels"] >= 0).sum(axis=1).tolist()
        print("%-24s e32 %.3e  settled %d / %d  exact ties outside sem1 %d  real nodes / smallest margin: %s"
              % (row["id"], e, int(ok.sum()), ok.numel(), exact_ties_outside_sem1(case["ref"]),
                 " ".join("%d/%.1e" % (f, m) for f, m in zip(fills, worst_margin.tolist()))), flush=True)
        if e > worst[0]:
            worst = (e, row["id"])
    print("e32 = %.3e (%s)  tau_plain = %.3e  tau_wide = %.3e" % (worst[0], worst[1], 16 * worst[0], 64 * worst[0]))
