"""sgpr_edgeconv_train_forward / _backward over the inputs training feeds them, called through the C-ABI with buffers
the test owns (so that the saved selection `sel` and `s1` = sum_k P_nbr can be read), against the tie-exact float64
reference tests/train_ref.pq_block_selected: exact ties in the max, hubs and repeated nodes in the lists, indices
outside [0, N), partial and mismatched channel tiles, batch and statistics edges, and the six blocks of a real step.

Every case is run twice, once on zero-filled outputs / scratch / workspace and once on NaN-filled ones (sel 255): the
two must agree bit for bit.  sel must equal the reference's choice exactly (both choose on the same fp32 P), s1 must lie
within one fp32 ulp of the float64 sum, and y, mean, var, dP, dQ, dgamma, dbeta meet test_gpu_edgeconv_train's RTOL /
ATOL, per channel."""
import numpy as np
import pytest
import torch

from test_gpu_edgeconv_train import ATOL, RTOL

pytestmark = pytest.mark.gpu

EPS = 1e-5
OUTS = ("y", "sel", "s1", "mean", "var", "dP", "dQ", "dgamma", "dbeta")
CHECKED = ("y", "mean", "var", "dP", "dQ", "dgamma", "dbeta")


# ---------------------------------------------------------------------------------------------------- the harness
def op(P, Q, idx, gamma, beta, dy, eps=EPS, dirty=False):
    """One forward and one backward through the C-ABI on GPU tensors (P, Q, dy [B,F,N] f32, idx [B,N,k] int64, gamma,
    beta [F] f32) -> {name: tensor}.  dirty: every output, d_dQ (the backward's scratch) and both workspaces start as NaN
    and sel as 255; otherwise all of them start as zeros."""
    from sg_pr_amd import engine
    from sg_pr_amd.train import ctypes_stream
    lib = engine.load_library()
    B, F, N = P.shape
    k = idx.shape[2]
    fill = float("nan") if dirty else 0.0

    def buf(*shape):
        return torch.full(shape, fill, dtype=torch.float32, device=P.device)

    out = {"y": buf(B, F, N), "s1": buf(B, F, N), "dP": buf(B, F, N), "dQ": buf(B, F, N)}
    for name in ("mean", "var", "dgamma", "dbeta"):
        out[name] = buf(F)
    out["sel"] = torch.full((B, F, N), 255 if dirty else 0, dtype=torch.uint8, device=P.device)
    ws_bytes = int(lib.sgpr_edgeconv_train_workspace_bytes(B, F))
    ws_f, ws_b = buf(ws_bytes // 4), buf(ws_bytes // 4)
    p, st = engine._ptr, ctypes_stream(P)
    rc = lib.sgpr_edgeconv_train_forward(p(P), p(Q), p(idx), p(gamma), p(beta), B, F, N, k, eps, p(out["y"]),
                                         p(out["sel"]), p(out["s1"]), p(out["mean"]), p(out["var"]), p(ws_f), ws_bytes,
                                         st)
    assert rc == 0, lib.sgpr_last_error().decode()
    rc = lib.sgpr_edgeconv_train_backward(p(dy), p(P), p(Q), p(idx), p(out["sel"]), p(out["s1"]), p(out["mean"]),
                                          p(out["var"]), p(gamma), p(beta), B, F, N, k, eps, p(out["dP"]), p(out["dQ"]),
                                          p(out["dgamma"]), p(out["dbeta"]), p(ws_b), ws_bytes, st)
    assert rc == 0, lib.sgpr_last_error().decode()
    torch.cuda.synchronize()
    return out


def reference(P, Q, idx, gamma, beta, dy, eps=EPS):
    """float64 autograd of train_ref.pq_block_selected on the same fp32 values -> {name: CPU tensor}."""
    from train_ref import pq_block_selected
    t = [v.detach().cpu().double().requires_grad_(True) for v in (P, Q, gamma, beta)]
    y, mean, var, sel, s1 = pq_block_selected(t[0], t[1], idx.cpu(), t[2], t[3], eps)
    y.backward(dy.detach().cpu().double())
    return {"y": y.detach(), "mean": mean.detach(), "var": var.detach(), "sel": sel, "s1": s1, "dP": t[0].grad,
            "dQ": t[1].grad, "dgamma": t[2].grad, "dbeta": t[3].grad}


def _per_channel(t):
    """[B,F,N] -> [F, B*N];  [F] -> [F, 1]"""
    return t.reshape(-1, 1) if t.dim() == 1 else t.transpose(0, 1).reshape(t.shape[1], -1)


def check(P, Q, idx, gamma, beta, dy, eps=EPS):
    """Run the op on clean and on dirty buffers, require the same bits, compare with the reference.
    -> (op outputs, reference)."""
    P, Q, dy = (v.float().cuda().contiguous() for v in (P, Q, dy))
    gamma, beta = gamma.float().cuda().contiguous(), beta.float().cuda().contiguous()
    idx = idx.to(device="cuda", dtype=torch.int64).contiguous()
    got = op(P, Q, idx, gamma, beta, dy, eps)
    dirty = op(P, Q, idx, gamma, beta, dy, eps, dirty=True)
    for name in OUTS:
        assert torch.equal(got[name], dirty[name]), "%s differs between zero- and NaN-filled buffers" % name
    ref = reference(P, Q, idx, gamma, beta, dy, eps)
    sel = got["sel"].cpu().long()
    bad = (sel != ref["sel"]).nonzero()
    assert bad.numel() == 0, "sel differs at %d of %d, first (b, f, i) %s: op %d, reference %d" % (
        bad.shape[0], sel.numel(), tuple(bad[0].tolist()), sel[tuple(bad[0])], ref["sel"][tuple(bad[0])])
    s1, s1r = got["s1"].cpu().double(), ref["s1"]
    a = s1r.abs().float()
    ulp = (torch.nextafter(a, torch.tensor(float("inf"))) - a).double()
    assert bool(((s1 - s1r).abs() <= ulp).all()), "s1: max |d| / ulp %g" % float(((s1 - s1r).abs() / ulp).max())
    for name in CHECKED:
        a, b = _per_channel(got[name].cpu().double()), _per_channel(ref[name].double())
        assert torch.isfinite(a).all(), name
        scale = b.abs().amax(dim=1)
        tol = ATOL * torch.clamp(scale, min=1.0) + RTOL * scale
        err = (a - b).abs().amax(dim=1)
        f = int(torch.argmax(err - tol))
        assert bool((err <= tol).all()), "%s: channel %d max |d| %g > tol %g (ref max %g)" % (
            name, f, float(err[f]), float(tol[f]), float(scale[f]))
    return got, ref


# ---------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def mixed_gamma(F, g):
    """|gamma| in [0.5, 1.5) with the sign cycling +, -, 0 over the channels."""
    ga = torch.rand(F, generator=g, dtype=torch.float64) + 0.5
    ga[1::3] *= -1.0
    ga[2::3] = 0.0
    return ga


def knn_lists(B, N, K, g):
    from sg_pr_amd import engine
    return engine.knn(torch.randn(B, 3, N, generator=g).cuda(), K)


def random_lists(B, N, K, g):
    return torch.randint(0, N, (B, N, K), generator=g)


def inputs(B, F, N, K, seed, lists=random_lists, quantised=False):
    """-> (P, Q, idx, gamma, beta, dy): continuous Q, beta, dy; P continuous or on the five levels -1 .. 1 in steps of
    0.5 (exact ties); gamma mixed."""
    g = _gen(seed)
    idx = lists(B, N, K, g)
    P = (torch.randint(-2, 3, (B, F, N), generator=g) * 0.5).double() if quantised else \
        torch.randn(B, F, N, generator=g, dtype=torch.float64)
    Q = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    ga = mixed_gamma(F, g)
    be = torch.randn(F, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    return P, Q, idx, ga, be, dy


def tied_rows(ref_key_P, idx, gamma):
    """Number of (b, f, i) whose best P is attained by more than one k."""
    b, f, n = ref_key_P.shape
    k = idx.shape[2]
    ix = idx.cpu().long().clamp(0, n - 1).reshape(b, 1, n * k).expand(b, f, n * k)
    Pn = torch.gather(ref_key_P.cpu().double(), 2, ix).view(b, f, n, k)
    key = torch.where(gamma.cpu().view(1, -1, 1, 1) < 0, -Pn, Pn)
    return int(((key == key.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1).sum())


def in_degree(idx):
    b, n, k = idx.shape
    ix = idx.cpu().long().clamp(0, n - 1)
    return torch.zeros(b, n, dtype=torch.int64).scatter_add_(1, ix.reshape(b, -1), torch.ones(b, n * k,
                                                                                            dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("B,F,N,K", [(16, 64, 100, 10), (4, 8, 1024, 64), (3, 65, 37, 37), (2, 100, 256, 20)])
def test_exact_ties_in_the_max(B, F, N, K):
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=B * 7 + F + K, lists=knn_lists, quantised=True)
    P[:, 3] = 0.75                                      # every row of channel 3 (gamma > 0) ties over all k
    P[:, 4] = -0.25                                     # and of channel 4 (gamma < 0)
    got, ref = check(P, Q, idx, ga, be, dy)
    assert bool((got["sel"][:, 3:5] == 0).all())
    assert tied_rows(P, idx, ga) >= B * F * N // 4       # the case really is full of ties


# ---------------------------------------------------------------------------------------------------- index lists
def semantic_graphs(B, N, seed, n_real_hi):
    """One-hot label features of packed synthetic graphs [B, 12, N], padded slots all zero (the semantic branch's
    layer-1 input), with at most n_real_hi <= N / 2 real nodes."""
    from sg_pr_amd import synth
    _, labels, _ = synth.make_graphs(B, N, max(1, n_real_hi // 3), n_real_hi, seed, kitti_like=True)
    lab = torch.from_numpy(labels).long()
    x = torch.nn.functional.one_hot(lab.clamp(min=0), 12).double() * (lab >= 0).unsqueeze(-1).double()
    return x.permute(0, 2, 1).contiguous()


@pytest.mark.parametrize("B,F,N,K", [(16, 64, 100, 10), (2, 32, 1024, 64)])
def test_knn_lists_of_padded_one_hot_graphs(B, F, N, K):
    """sgpr_knn on identical columns picks the lowest indices: every padded row lists the same k padded slots."""
    from sg_pr_amd import engine
    x = semantic_graphs(B, N, seed=N + K, n_real_hi=N // 2)
    idx = engine.knn(x.float().cuda(), K)
    assert int(in_degree(idx).max()) >= 4 * K
    g = _gen(K)
    wa = torch.randn(F, 12, generator=g, dtype=torch.float64)
    wq = torch.randn(F, 12, generator=g, dtype=torch.float64)
    P, Q = torch.matmul(wa, x), torch.matmul(wq, x) + 0.1 * torch.randn(B, F, N, generator=g, dtype=torch.float64)
    ga = mixed_gamma(F, g)
    be = torch.randn(F, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    check(P, Q, idx, ga, be, dy)
    assert tied_rows(P.float(), idx, ga) > 0


@pytest.mark.parametrize("B,F,N,K", [(8, 16, 100, 10), (2, 8, 37, 37), (4, 64, 256, 20)])
def test_repeated_nodes_within_a_row(B, F, N, K):
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=3 * K + F)
    g = _gen(N)
    idx[:, ::2, 1::2] = idx[:, ::2, 0:K - 1:2]                    # even rows: every pair of slots lists one node twice
    idx[:, 1::4] = torch.randint(0, 3, (B, idx[:, 1::4].shape[1], K), generator=g)   # some rows use only 3 nodes
    rows = [set(r.tolist()) for r in idx.reshape(-1, K)]
    assert sum(len(r) < K for r in rows) >= B * N // 2
    check(P, Q, idx, ga, be, dy)


@pytest.mark.parametrize("B,F,N,K,quantised", [(2, 8, 256, 20, False), (2, 8, 256, 20, True), (2, 2, 1024, 64, False)])
def test_one_hub_receives_every_edge(B, F, N, K, quantised):
    """Every edge of a graph lands on one node: in-degree N k (65 536, the whole 16-bit edge list, at N = 1024, k = 64;
    the backward's bucket sort takes ~0.3 s there on the MI355X, against 0.4 ms for random lists).  Two graphs: with
    one, the hub's dP is exactly 0 (G_j = dbeta, indeg_j = M) and the op returns the fp32 residue of G_j - M dbeta / M,
    ~1e-6 of the ~30 those terms measure at N = 1024, which RTOL / ATOL relative to a zero result cannot express."""
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=11, quantised=quantised)
    for b in range(B):
        idx[b] = (5, N - 1)[b % 2]
    got, _ = check(P, Q, idx, ga, be, dy)
    assert bool((got["sel"] == 0).all())
    assert int(in_degree(idx).max()) == N * K


def test_out_of_range_indices_are_clamped():
    B, F, N, K = 4, 16, 100, 10
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=5, quantised=True)
    g = _gen(6)
    idx = torch.randint(-2 * N, 2 * N, (B, N, K), generator=g)
    idx[0, 0] = torch.tensor([-1, N, -2 ** 40, 2 ** 40, -2 ** 63, 2 ** 63 - 1, 0, N - 1, N + 1, -N])
    got, _ = check(P, Q, idx, ga, be, dy)
    clamped = check(P, Q, idx.clamp(0, N - 1), ga, be, dy)[0]
    for name in OUTS:
        assert torch.equal(got[name], clamped[name]), name


# ---------------------------------------------------------------------------------------------------- channel tiles
@pytest.mark.parametrize("B,F,N,K", [(4, 65, 100, 10), (4, 100, 100, 10), (4, 130, 100, 10), (2, 257, 100, 10),
                                     (3, 20, 1000, 20), (2, 24, 1024, 1), (2, 40, 512, 9)])
def test_partial_and_mismatched_channel_tiles(B, F, N, K):
    """F past one 64-wide tile with the last one partial; at N = 1000 the stats tile is 8 wide (the last one 4 of 8);
    at (1024, 1) and (512, 9) the scatter tile (16, 32) is wider than the stats tile (8, 16)."""
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=F + N + K, quantised=bool(F % 2))
    check(P, Q, idx, ga, be, dy)


# ---------------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("B,F,N,K", [(1, 8, 100, 10), (4096, 2, 8, 4), (70000, 1, 4, 2)])
def test_batch_edges(B, F, N, K):
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=B + K, quantised=B > 1000)
    if F == 1:
        ga[0] = -0.8
    check(P, Q, idx, ga, be, dy)


def test_single_edge():
    """N = k = 1, B = 1: one edge per channel, variance 0, y = LeakyReLU(beta) exactly; only beta has a gradient."""
    g = _gen(9)
    P, Q = torch.randn(1, 4, 1, generator=g) * 3, torch.randn(1, 4, 1, generator=g) * 3
    ga = torch.tensor([1.0, -1.0, 0.0, 2.0])
    be = torch.tensor([0.5, -0.5, 0.25, -2.0])
    dy = torch.randn(1, 4, 1, generator=g)
    got, _ = check(P, Q, torch.zeros(1, 1, 1, dtype=torch.int64), ga, be, dy)
    assert torch.equal(got["y"].cpu().view(-1), torch.nn.functional.leaky_relu(be, 0.2))
    # var = E[z^2] - mean^2 from the expanded per-node sums P^2 + 2 P Q + Q^2 in fp64: up to ~4 (|P| + |Q|)^2 2^-53
    # of rounding instead of 0, far below eps (y above is exact: z - mean is 0 in fp32)
    assert float(got["var"].abs().max()) <= 4 * float((P.abs() + Q.abs()).max()) ** 2 * 2.0 ** -53
    assert float(got["dP"].abs().max()) == 0.0 and float(got["dQ"].abs().max()) == 0.0
    assert float(got["dgamma"].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- statistics
def test_constant_channels():
    """Channel 0: z = 1 on every edge (P = 0.75, Q = 0.25: the sums are exact, var = 0, every row ties); channel 1: P
    constant, Q continuous; channel 2: Q constant, P continuous."""
    B, F, N, K = 4, 6, 100, 10
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=21, lists=knn_lists)
    P[:, 0], Q[:, 0] = 0.75, 0.25
    P[:, 1] = -1.5
    Q[:, 2] = 2.0
    got, _ = check(P, Q, idx, ga, be, dy)
    assert float(got["var"][0]) == 0.0 and float(got["mean"][0]) == 1.0
    assert bool((got["sel"][:, :2] == 0).all())


def test_large_common_offset():
    """z = 1000 + N(0, 1): P = 500 + N(0, 0.5), Q = 500 + N(0, 0.5).  The op rounds z = Q + P and mean to fp32: each
    carries |z| 2^-24 ~ 6e-5 of absolute error, 6e-5 of xhat at sigma ~ 1, below RTOL * |y| ~ 2e-4 at |y| ~ 1; mean
    ~ 1000 is held to RTOL relative.  No tolerance beyond RTOL / ATOL."""
    B, F, N, K = 8, 8, 100, 10
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=31, lists=knn_lists)
    P, Q = 500.0 + 0.5 * P, 500.0 + 0.5 * Q
    got, ref = check(P, Q, idx, ga, be, dy)
    assert float(ref["mean"].min()) > 990.0 and 0.3 < float(ref["var"].min()) and float(ref["var"].max()) < 1.0


def test_cancelling_layer_one_regime():
    """The xyz branch's first layer: P and Q both ~ 50 m of opposite sign, z = P + Q of order sigma.  z itself is exact
    (Sterbenz: P and -Q within a factor 2), but s1 = sum_k P (|s1| <= k |P|) and the fp32 terms S1 + k Q - k mean (dQ)
    and indeg (P_j - mean) + R_j (dP) carry up to ~3 k |P| 2^-24 of absolute error, which the BN backward divides by
    sigma and by M / dgamma.  Relative to the O(sigma) size of those terms that is 3 k |P| 2^-24 / sigma; here
    3 * 10 * 52 * 2^-24 / 0.5 ~ 1.9e-4 of a term that enters dQ / dP scaled by dgamma / M << 1, so RTOL / ATOL hold."""
    B, F, N, K = 16, 16, 100, 10
    P, Q, idx, ga, be, dy = inputs(B, F, N, K, seed=41, lists=knn_lists)
    P, Q = 50.0 + 0.5 * P, -50.0 + 0.5 * Q
    sigma = 0.5 * np.sqrt(2.0)
    bound = 3 * K * float(P.abs().max()) * 2.0 ** -24 / sigma
    assert bound < RTOL
    got, ref = check(P, Q, idx, ga, be, dy)
    assert float(ref["mean"].abs().max()) < 0.5


# ---------------------------------------------------------------------------------------------------- recorded inputs
def test_recorded_inputs_of_a_training_step(oracle_sd, monkeypatch):
    """The six EdgeConv blocks of one train_loss(...).backward() on the golden + synthetic graphs, their (P, Q, idx,
    gamma, beta, dy) recorded as the step ran, each replayed through the harness and checked against the reference."""
    from sg_pr_amd import train
    from test_gpu_train_step import _golden_plus_synth, _model
    real = train.EdgeConvBN
    rec = []

    class Recorder:
        @staticmethod
        def apply(P, Q, idx, gamma, beta, eps):
            e = {"P": P.detach().float().contiguous().clone(), "Q": Q.detach().float().contiguous().clone(),
                 "idx": idx.detach().clone(), "gamma": gamma.detach().float().clone(),
                 "beta": beta.detach().float().clone(), "eps": float(eps)}
            y, mean, var = real.apply(P, Q, idx, gamma, beta, eps)
            e["y"] = y.detach().clone()
            y.register_hook(lambda g, e=e: e.__setitem__("dy", g.detach().float().contiguous().clone()))
            rec.append(e)
            return y, mean, var

    monkeypatch.setattr(train, "EdgeConvBN", Recorder)
    centers, labels = _golden_plus_synth(13)
    feats = train.dense_features(torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda())
    target = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0], device="cuda")
    model = _model(oracle_sd)
    loss, _, _ = train.train_loss(model, feats, target)
    loss.backward()
    torch.cuda.synchronize()
    assert len(rec) == 6 and all("dy" in e for e in rec)
    for j, e in enumerate(rec):
        got, _ = check(e["P"], e["Q"], e["idx"], e["gamma"], e["beta"], e["dy"], e["eps"])
        assert torch.equal(got["y"], e["y"]), "block %d: the harness is not the op EdgeConvBN ran" % j
        if j >= 3:    # the semantic branch: one-hot labels and padded slots make exact ties in P
            assert tied_rows(e["P"], e["idx"], e["gamma"]) > 0, j
