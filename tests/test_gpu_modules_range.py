"""The stand-alone modules (dgcnn.knn / get_graph_feature, AttentionModule, TenorNetworkModule; include/sgpr.h) over the
range their entry points promise - N <= 1024, k <= 64, F <= 128, T <= 64, empty batches - against float64 references of
the same operations, with bounds derived from each output's own terms.  test_gpu_modules.py holds the reference goldens
at the shipped shape.  `pytest -m gpu`."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -23              # twice fp32's unit roundoff
LDS_BYTES = 160 * 1024      # one workgroup's LDS: the LDS-resident kNN instance takes a graph only below it


def _lds_instance(C, N, k):
    """Does sgpr_knn take the LDS-resident instance (sgpr_modules.hip) for this shape, or the wave-per-row one?"""
    return N <= 256 and k <= 32 and (((C + 1) * N * 4 + 7) & ~7) + k * 256 * 8 <= LDS_BYTES


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- kNN
def _knn_distinct(idx, N):
    assert ((idx >= 0) & (idx < N)).all()
    s = idx.sort(-1)[0]
    assert (s[..., 1:] != s[..., :-1]).all(), "a row repeats a candidate"


def _knn_check(x, k, idx, finite=None):
    """idx [B,N,k] against float64 |xi - xj|^2: k distinct candidates per row, best first, and the k nearest - a selected
    and an excluded candidate may trade places only if their distances lie within the rounding bound of the fp32 keys,
    (C + 4) 2^-23 (|xi|^2 + |xj|^2) each.  finite [B,N] bool: only those nodes' rows are checked, over those candidates."""
    B, C, N = x.shape
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (B, N, k)
    _knn_distinct(idx, N)
    xd = x.double()
    if finite is not None:
        xd = torch.where(finite[:, None, :], xd, torch.zeros_like(xd))
    xx = (xd * xd).sum(1)
    d = (xx[:, :, None] + xx[:, None, :] - 2.0 * xd.transpose(1, 2) @ xd).clamp_min(0.0)
    err = (C + 4) * U * (xx[:, :, None] + xx[:, None, :])
    if finite is not None:
        d = d.masked_fill(~finite[:, None, :], float("inf"))
        err = err.masked_fill(~finite[:, None, :], 0.0)
    ds, es = d.gather(2, idx), err.gather(2, idx)
    rows = torch.ones(B, N, dtype=torch.bool) if finite is None else finite
    order_ok = ((ds[..., :-1] - ds[..., 1:]) <= es[..., :-1] + es[..., 1:]).all(-1)
    assert order_ok[rows].all(), "a row is not nearest first"
    sel = torch.zeros(B, N, N, dtype=torch.bool).scatter_(2, idx, True)
    worst_in = (ds - es).amax(-1)
    best_out = (d + err).masked_fill(sel, float("inf")).amin(-1)
    bad = (worst_in > best_out) & rows
    assert not bad.any(), "rows whose set is not the k nearest: %d, first %s" % (bad.sum(), bad.nonzero()[0].tolist())


KNN_SHAPES = [  # (B, C, N, k)
    (3, 3, 1, 1), (3, 1, 2, 2), (1, 3, 2, 1), (3, 12, 63, 10), (1, 64, 64, 32), (3, 3, 65, 20), (1, 256, 63, 1),
    (3, 128, 232, 20), (3, 128, 240, 20), (1, 128, 256, 20), (3, 256, 128, 10), (1, 256, 128, 20), (3, 1, 255, 32),
    (3, 3, 256, 32), (3, 64, 64, 64), (1, 12, 33, 33), (3, 3, 257, 10), (1, 64, 511, 33), (3, 12, 1024, 64),
    (1, 256, 1024, 20), (1, 1, 1024, 1), (1, 3, 511, 64),
]


@pytest.mark.parametrize("B,C,N,k", KNN_SHAPES,
                         ids=["B%d-C%d-N%d-k%d-%s" % (s + ("lds" if _lds_instance(*s[1:]) else "wave",)) for s in KNN_SHAPES])
def test_knn_is_the_float64_k_nearest(B, C, N, k):
    from sg_pr_amd import dgcnn
    x = torch.randn(B, C, N, generator=_gen(1000 * C + N + k))
    idx = dgcnn.knn(x.cuda(), k).cpu()
    _knn_check(x, k, idx)


def test_knn_lds_limit_straddles_the_documented_shapes():
    """The shapes above do fall on both sides of the LDS-resident instance's limit (C = 128, N = 256, k = 20 - the
    second EdgeConv input of a filters-128 model - is beyond it and is served, not refused)."""
    assert _lds_instance(128, 232, 20) and not _lds_instance(128, 240, 20) and not _lds_instance(128, 256, 20)
    assert _lds_instance(256, 128, 10) and not _lds_instance(256, 128, 20)


@pytest.mark.parametrize("n,k,g", [(256, 20, 64), (100, 10, 160), (512, 20, 32), (1024, 64, 16)])
def test_knn_coordinate_lists_are_the_reference_fp32_keys(oracle, n, k, g):
    """C = 3, centres spread like a scene: the neighbour sets are the reference's own fp32 keys (dgcnn.py:14-20,
    oracle.neg_sq_dist) with no allowance - both instances restate that expansion operation for operation.  Compared
    through the key values, which is indifferent to the order among exactly equal keys."""
    from sg_pr_amd import dgcnn
    x = (torch.rand(g, 3, n, generator=_gen(n + k)) * 200.0 - 100.0)
    x[:, 1] *= 0.1
    idx = dgcnn.knn(x.cuda(), k).cpu()
    _knn_distinct(idx, n)
    pd = oracle.neg_sq_dist(x)
    ref = pd.topk(k, dim=-1)[0].sort(-1)[0]
    got = pd.gather(2, idx).sort(-1)[0]
    bad = (ref != got).any(-1)
    assert not bad.any(), "rows off the reference's fp32 keys: %d of %d" % (bad.sum(), bad.numel())
    _knn_check(x, k, idx)           # best first (in order only within rounding: torch's own products may round otherwise)


def _tie_data(B, C, N, seed):
    """Small-integer coordinates with the second half of the nodes a copy of the first: many exactly equal keys, and
    every key exact in fp32."""
    x = torch.randint(-2, 3, (B, C, N), generator=_gen(seed)).float()
    h = N // 2
    x[:, :, N - h:] = x[:, :, :h]
    return x


@pytest.mark.parametrize("B,C,N", [(3, 1, 64), (3, 3, 100), (2, 12, 256), (4, 64, 33), (3, 3, 256), (1, 128, 150)])
def test_knn_instances_return_identical_lists(B, C, N):
    """knn(x, k) with k <= 32 on the LDS-resident instance is, bit for bit, the head of knn(x, 33) on the wave-per-row
    instance: the same keys (knn_key) under the same order (knn_rank).  On exact small-integer data the lists are also
    the exact (distance, index) order."""
    from sg_pr_amd import dgcnn
    for data in ("random", "ties"):
        x = torch.randn(B, C, N, generator=_gen(N + C)) if data == "random" else _tie_data(B, C, N, N + C)
        xg = x.cuda()
        full = dgcnn.knn(xg, 33)
        for k in (1, 10, 20, 32):
            assert _lds_instance(C, N, k)
            got = dgcnn.knn(xg, k)
            assert torch.equal(got, full[..., :k]), (data, k)
        if data == "ties":
            xd = x.double()
            d = ((xd[:, :, :, None] - xd[:, :, None, :]) ** 2).sum(1)          # exact: integers
            want = torch.sort(d, dim=-1, stable=True)[1][..., :33]
            assert torch.equal(full.cpu(), want)
        else:
            _knn_check(x, 33, full.cpu())


@pytest.mark.parametrize("N,C", [(64, 3), (100, 12), (300, 3)])
def test_knn_non_finite_nodes_rank_last(N, C):
    """A NaN node and a 1e30 node (|x|^2 overflows: +inf and NaN keys) at low, middle and last indices: rows of finite
    nodes hold the k nearest finite nodes, no non-finite candidate ranks ahead of a finite one in any row but the NaN
    node's own, every row holds k distinct indices, and both instances return the same lists."""
    from sg_pr_amd import dgcnn
    places = [(0, 1), (1, 0), (N // 2, N // 2 + 1), (N - 1, N - 2), (N - 2, N - 1), (N // 3, 0)]
    B = len(places)
    x = torch.randn(B, C, N, generator=_gen(N * C))
    finite = torch.ones(B, N, dtype=torch.bool)
    for b, (pn, pb) in enumerate(places):
        x[b, :, pn] = float("nan")
        x[b, :, pb] = 1e30
        finite[b, pn] = finite[b, pb] = False
    xg = x.cuda()
    ks = (10, 32) if N <= 256 else (10, 64)
    lists = {k: dgcnn.knn(xg, k).cpu() for k in ks + (33,)}
    for k, idx in lists.items():
        _knn_check(x, k, idx, finite=finite)                             # (every row: k distinct indices)
        fin = finite.gather(1, idx.view(B, -1)).view(B, N, k)
        for b, (pn, pb) in enumerate(places):
            rows = torch.arange(N) != pn
            # a finite candidate never follows a non-finite one
            assert not (~fin[b, rows, :-1] & fin[b, rows, 1:]).any(), (k, b)
            assert fin[b, finite[b], :].all(), (k, b)             # >= k finite nodes exist: only finite ones taken
    full = lists[33]
    for k in ks:
        if k <= 32 and N <= 256:
            assert torch.equal(lists[k], full[..., :k]), k


def test_knn_more_graphs_than_one_grid_dimension():
    """65 537 graphs on the wave instance (N = 257): launch_knn_any splits grid.y at 65 535.  Every graph's coordinates are
    its own permutation of 0..256, so the answer is known: the node itself, then the lower-indexed of the nodes one
    below and one above it (the ends have one)."""
    from sg_pr_amd import dgcnn
    B, N = 65537, 257
    perm = torch.argsort(torch.rand(B, N, device="cuda"), dim=1)
    x = perm.float().unsqueeze(1)                                          # [B, 1, N]: value of node n = perm[b, n]
    idx = dgcnn.knn(x, 2)
    assert tuple(idx.shape) == (B, N, 2)
    pos = torch.argsort(perm, dim=1)                                       # pos[b, v] = node holding value v
    INF = N + 1
    below = torch.cat((torch.full((B, 1), INF, device="cuda"), pos[:, :-1]), 1)     # node of value v - 1
    above = torch.cat((pos[:, 1:], torch.full((B, 1), INF, device="cuda")), 1)      # node of value v + 1
    want_v = torch.minimum(below, above)                                   # indexed by value
    want = want_v.gather(1, perm)                                          # indexed by node
    assert torch.equal(idx[..., 0], torch.arange(N, device="cuda").expand(B, N))
    assert torch.equal(idx[..., 1], want)


def test_knn_empty_batch():
    from sg_pr_amd import dgcnn
    for C, N, k in ((3, 10, 5), (128, 256, 20), (3, 1024, 64)):
        idx = dgcnn.knn(torch.empty(0, C, N, device="cuda"), k)
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (0, N, k)


# ------------------------------------------------------------------------------------------------------ graph feature
def _gather(x, idx):
    """cat(x_j - x_i, x_i) [B,2C,N,k] by torch indexing on the device."""
    B, C, N = x.shape
    k = idx.shape[2]
    xt = x.transpose(1, 2)                                                 # [B,N,C]
    nb = xt[torch.arange(B, device=x.device)[:, None, None], idx]          # [B,N,k,C]
    nb = nb.permute(0, 3, 1, 2)
    ctr = x[:, :, :, None].expand(B, C, N, k)
    return torch.cat((nb - ctr, ctr), dim=1)


@pytest.mark.parametrize("B,C,N,k", [(3, 3, 1, 1), (3, 12, 63, 10), (1, 256, 64, 64), (3, 128, 257, 20),
                                     (1, 64, 1024, 64), (3, 1, 1024, 33), (1, 256, 1024, 64), (3, 3, 5, 40)])
def test_graph_feature_is_the_torch_gather(B, C, N, k):
    from sg_pr_amd import dgcnn
    x = torch.randn(B, C, N, generator=_gen(C * N + k)).cuda()
    rnd = torch.randint(0, N, (B, N, k), generator=_gen(k)).cuda()
    rnd[..., 0] = 0
    rnd[..., -1] = N - 1
    lists = [rnd]
    if k <= min(N, 64):
        lists.append(dgcnn.knn(x, k))
    for idx in lists:
        got = dgcnn.get_graph_feature(x, k=k, idx=idx)
        assert tuple(got.shape) == (B, 2 * C, N, k)
        assert torch.equal(got, _gather(x, idx))


def test_graph_feature_clamps_out_of_range_indices():
    """include/sgpr.h: an index outside [0, N) reads the nearest end of the graph - no read leaves it."""
    from sg_pr_amd import dgcnn
    B, C, N, k = 3, 5, 40, 8
    x = torch.randn(B, C, N, generator=_gen(5)).cuda()
    idx = torch.randint(0, N, (B, N, k), generator=_gen(6))
    idx[..., 1], idx[..., 2], idx[..., 3], idx[..., 4] = -1, -(2 ** 40), N, 2 ** 40
    idx = idx.cuda()
    assert torch.equal(dgcnn.get_graph_feature(x, k=k, idx=idx), _gather(x, idx.clamp(0, N - 1)))


def test_graph_feature_empty_batch():
    from sg_pr_amd import dgcnn
    for C, N, k in ((3, 10, 5), (256, 1024, 64)):
        out = dgcnn.get_graph_feature(torch.empty(0, C, N, device="cuda"), k=k,
                                      idx=torch.empty(0, N, k, dtype=torch.int64, device="cuda"))
        assert tuple(out.shape) == (0, 2 * C, N, k)
    assert tuple(dgcnn.get_graph_feature(torch.empty(0, 3, 10, device="cuda"), k=4).shape) == (0, 6, 10, 4)


# -------------------------------------------------------------------------------------------------------- attention
def _args(**kw):
    from sg_pr_amd.parser_sg import sgpr_args
    a = sgpr_args()
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def _attention_ref(oracle, w, emb):
    """oracle.attention in float64 and, per output, a bound c 2^-23 sum|terms| with c = N + F + 8 (the longest sum on the
    way plus the width), its terms propagated through the mean, the context, the sigmoid and the weighted sum."""
    B, N, F = emb.shape
    wd, ed = w.double(), emb.double()
    rep, sig = oracle.attention({"attention.weight_matrix": wd}, ed)
    rep, sig = rep.squeeze(-1), sig.squeeze(-1)                            # [B,F], [B,N]
    c = (N + F + 8) * U
    ea = ed.abs()
    ctx = torch.tanh(ed.mean(1) @ wd)                                      # [B,F]
    s_g = ea.mean(1) @ wd.abs()                                            # terms of the context's argument
    s_d = torch.einsum("bnf,bf->bn", ea, ctx.abs() + s_g)                 # terms of each score's argument
    att_tol = c * (0.25 * s_d + 1.0)
    rep_tol = c * torch.einsum("bnf,bn->bf", ea, sig + 0.25 * s_d + 1.0)
    return rep, sig, rep_tol, att_tol


ATT_F = [1, 16, 31, 32, 33, 64, 128]
ATT_N = [1, 7, 255, 256, 257, 1000, 12288, 12289]


@pytest.mark.parametrize("F", ATT_F)
def test_attention_module_is_the_float64_reference(oracle, F):
    """F below, at and above the built width (zero-padded, tuned, any-width kernel) and N across the any-width kernel's
    256-node chunks and the tuned kernel's 12 288-node limit (beyond it the any-width kernel serves every F)."""
    from sg_pr_amd.layers_batch import AttentionModule
    torch.manual_seed(F)
    mod = AttentionModule(_args(filters_3=F)).cuda().eval()
    w = mod.weight_matrix.detach().cpu()
    for N in ATT_N:
        B = 5 if N <= 1000 else 1
        emb = torch.randn(B, N, F, generator=_gen(N + F)) + 0.25
        with torch.no_grad():
            rep, att = mod(emb.cuda())
        assert tuple(rep.shape) == (B, F, 1) and tuple(att.shape) == (B, N, 1)
        ref_rep, ref_att, rep_tol, att_tol = _attention_ref(oracle, w, emb)
        d_att = (att.squeeze(-1).cpu().double() - ref_att).abs()
        d_rep = (rep.squeeze(-1).cpu().double() - ref_rep).abs()
        assert (d_att <= att_tol).all(), (N, (d_att / att_tol).max().item())
        assert (d_rep <= rep_tol).all(), (N, (d_rep / rep_tol).max().item())
    with torch.no_grad():
        rep, att = mod(torch.empty(0, 7, F, device="cuda"))
    assert tuple(rep.shape) == (0, F, 1) and tuple(att.shape) == (0, 7, 1)


def test_attention_without_scores_gives_the_same_representation():
    """d_att = NULL (the scores not wanted) leaves d_rep bit for bit what it is with them, on both kernels."""
    from sg_pr_amd import engine
    lib = engine.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
    for F, N in ((32, 300), (32, 12288), (64, 1000), (7, 257)):
        B = 3
        emb = torch.randn(B, N, F, generator=_gen(F * N)).cuda()
        w = (torch.randn(F, F, generator=_gen(F)) * 0.2).cuda()
        reps = []
        for want_att in (True, False):
            rep = torch.full((B, F), float("nan"), device="cuda")
            att = torch.empty(B, N, device="cuda") if want_att else None
            if F == 32:
                rc = lib.sgpr_attention_pool(p(w), p(emb), B, N, p(rep), p(att), None)
            else:
                rc = lib.sgpr_attention_pool_any(p(w), p(emb), B, N, F, p(rep), p(att), None)
            assert rc == 0, lib.sgpr_last_error()
            torch.cuda.synchronize()
            reps.append(rep)
        assert torch.equal(reps[0], reps[1]), (F, N)
        assert torch.isfinite(reps[0]).all()


# -------------------------------------------------------------------------------------------------------------- NTN
NTN_SHAPES = [(32, 16), (8, 4), (31, 16), (32, 15), (33, 16), (32, 17), (1, 1), (128, 64)]


@pytest.mark.parametrize("F,T", NTN_SHAPES)
def test_tensor_network_module_is_the_float64_reference(oracle, F, T):
    """The built shape (tuned kernel, 4 pairs a block: B = 5 leaves a tail), smaller modules (zero-padded into it) and
    wider ones (any-width kernel, 4 096 blocks: B = 4 097 strides past them) against oracle.tensor_network in float64,
    per output within c 2^-23 sum|terms|, c = 2F + 16."""
    from sg_pr_amd.layers_batch import TenorNetworkModule
    torch.manual_seed(100 * F + T)
    mod = TenorNetworkModule(_args(filters_3=F, tensor_neurons=T)).cuda().eval()
    w, wb, bias = (p.detach().cpu().double() for p in (mod.weight_matrix, mod.weight_matrix_block, mod.bias))
    sd = {"tensor_network.weight_matrix": w, "tensor_network.weight_matrix_block": wb, "tensor_network.bias": bias}
    for B in (0, 1, 5, 4097):
        e1 = torch.randn(B, F, 1, generator=_gen(B + F))
        e2 = torch.randn(B, F, 1, generator=_gen(B + T + 1)) + 0.5
        with torch.no_grad():
            out = mod(e1.cuda(), e2.cuda())
        assert tuple(out.shape) == (B, T, 1)
        if B == 0:
            continue
        e1d, e2d = e1.double(), e2.double()
        ref = oracle.tensor_network(sd, e1d, e2d).squeeze(-1)
        terms = (torch.einsum("bi,ijt,bj->bt", e1d.abs().squeeze(-1), w.abs(), e2d.abs().squeeze(-1)) +
                 (wb.abs() @ torch.cat((e1d, e2d), 1).abs()).squeeze(-1) + bias.abs().view(1, T))
        tol = (2 * F + 16) * U * terms
        d = (out.squeeze(-1).cpu().double() - ref).abs()
        assert (d <= tol).all(), (B, (d / tol).max().item())
