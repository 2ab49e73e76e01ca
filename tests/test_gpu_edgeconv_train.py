"""sgpr_edgeconv_train_forward / _backward (EdgeConvBN) against float64 autograd of the dense formulation
(tests/train_ref.pq_block) on continuous random inputs; kNN lists come from sgpr_knn."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# fp32 kernel vs fp64 reference: values are O(1), the batch statistics sum up to ~10^6 edges in fp64 and per-node sums in
# fp32 over <= 64 terms; dP sums up to ~N * k terms of O(1 / M)
RTOL, ATOL = 2e-4, 2e-5


def _case(B, F, N, K, seed, gamma=None):
    from sg_pr_amd import engine
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, N, generator=g).cuda()
    idx = engine.knn(x, K)
    P = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    Q = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    ga = torch.rand(F, generator=g, dtype=torch.float64) + 0.5 if gamma is None else gamma.double()
    be = torch.randn(F, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    return idx, P, Q, ga, be, dy


def _run(idx, P, Q, ga, be, dy):
    from sg_pr_amd.train import EdgeConvBN
    t = [v.float().cuda().requires_grad_(True) for v in (P, Q, ga, be)]
    y, mean, var = EdgeConvBN.apply(t[0], t[1], idx, t[2], t[3], 1e-5)
    y.backward(dy.float().cuda())
    return [v.detach().cpu().double() for v in (y, mean, var)] + [v.grad.cpu().double() for v in t]


def _ref(idx, P, Q, ga, be, dy):
    from train_ref import pq_block
    t = [v.clone().requires_grad_(True) for v in (P, Q, ga, be)]
    y, mean, var = pq_block(t[0], t[1], idx.cpu(), t[2], t[3], 1e-5)
    y.backward(dy)
    return [y.detach(), mean.detach(), var.detach()] + [v.grad for v in t]


NAMES = ("y", "mean", "var", "dP", "dQ", "dgamma", "dbeta")


def _compare(got, ref, scale_grad=True):
    for name, a, b in zip(NAMES, got, ref):
        tol = ATOL * max(1.0, float(b.abs().max())) if b.numel() else ATOL
        err = float((a - b).abs().max()) if b.numel() else 0.0
        assert err <= tol + RTOL * float(b.abs().max()), "%s: max |d| %g (ref max %g)" % (name, err, float(b.abs().max()))


SHAPES = [  # (B, F, N, K): the six layer shapes of the shipped model (C = 3 / 12 / 64 feed F = 64 / 32), then the range
    (16, 64, 100, 10), (16, 32, 100, 10),
    (4, 64, 256, 20), (2, 16, 1024, 64),
    (1, 8, 100, 10), (4, 8, 100, 1), (2, 8, 37, 37), (3, 1, 100, 10), (5, 12, 37, 10),
]


@pytest.mark.parametrize("B,F,N,K", SHAPES)
def test_forward_backward_vs_float64(B, F, N, K):
    case = _case(B, F, N, K, seed=B * 1000 + F * 10 + K)
    _compare(_run(*case), _ref(*case))


@pytest.mark.parametrize("C,F", [(3, 64), (12, 64), (64, 64), (64, 32)])
def test_layer_shapes_through_the_block(C, F):
    """edgeconv_block of the shipped layer shapes: dW and dx through torch's GEMMs against the dense edge tensor."""
    from sg_pr_amd.train import edgeconv_block
    from train_ref import edge_block
    torch.manual_seed(C + F)
    blk = torch.nn.Sequential(torch.nn.Conv2d(2 * C, F, 1, bias=False), torch.nn.BatchNorm2d(F),
                              torch.nn.LeakyReLU(0.2)).cuda()
    x = torch.randn(8, C, 100, device="cuda", requires_grad=True)
    y, idx = edgeconv_block(x, blk, 10, updates=0)
    dy = torch.randn_like(y)
    y.backward(dy)
    xr = x.detach().cpu().double().requires_grad_(True)
    w = blk[0].weight.detach().cpu().double().requires_grad_(True)
    ga = blk[1].weight.detach().cpu().double().requires_grad_(True)
    be = blk[1].bias.detach().cpu().double().requires_grad_(True)
    yr, _, _ = edge_block(xr, idx.cpu(), w.view(F, 2 * C), ga, be)
    yr.backward(dy.cpu().double())
    for a, b in ((y, yr), (x.grad, xr.grad), (blk[0].weight.grad, w.grad), (blk[1].weight.grad, ga.grad),
                 (blk[1].bias.grad, be.grad)):
        a, b = a.detach().cpu().double(), b.detach()
        assert float((a - b).abs().max()) <= 5e-4 * max(1.0, float(b.abs().max()))


def test_negative_and_zero_gamma():
    B, F, N, K = 6, 8, 100, 10
    gamma = torch.tensor([1.0, -0.7, 0.0, -2.0, 0.5, 0.0, -0.1, 1.5])
    idx, P, Q, ga, be, dy = _case(B, F, N, K, seed=7, gamma=gamma)
    got, ref = _run(idx, P, Q, ga, be, dy), _ref(idx, P, Q, ga, be, dy)
    nz = gamma != 0
    for name, a, b in zip(NAMES, got, ref):
        if name == "dgamma":      # at gamma = 0 every edge ties: the op takes the gamma -> 0+ side (the largest P)
            a, b = a[nz], b[nz]
        assert float((a - b).abs().max()) <= ATOL + RTOL * max(1.0, float(b.abs().max())), name
    # gamma = 0: y = LReLU(beta), no gradient reaches P or Q through the channel; dgamma from the largest-P edge
    z = torch.gather(P, 2, idx.cpu().reshape(B, 1, N * K).expand(B, F, N * K)).view(B, F, N, K) + Q.unsqueeze(-1)
    mu, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
    Pn = torch.gather(P, 2, idx.cpu().reshape(B, 1, N * K).expand(B, F, N * K)).view(B, F, N, K)
    ks = Pn.argmax(dim=-1, keepdim=True)
    xh = (torch.gather(z, 3, ks).squeeze(-1) - mu.view(1, -1, 1)) / torch.sqrt(var.view(1, -1, 1) + 1e-5)
    gz = dy * torch.where(be.view(1, -1, 1) > 0, 1.0, 0.2)
    want = (gz * xh).sum(dim=(0, 2))
    for f in np.nonzero((~nz).numpy())[0]:
        assert abs(float(got[5][f]) - float(want[f])) <= 1e-3 * max(1.0, abs(float(want[f])))
        assert float(got[3][:, f].abs().max()) == 0.0 and float(got[4][:, f].abs().max()) == 0.0


def test_bitwise_repeatable_dirty_buffers_and_streams():
    from sg_pr_amd.train import EdgeConvBN
    idx, P, Q, ga, be, dy = _case(8, 64, 100, 10, seed=3)
    first = _run(idx, P, Q, ga, be, dy)
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 22,), float("nan"), device="cuda") for _ in range(4)]   # the next allocations hold NaN
    del junk
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again = _run(idx, P, Q, ga, be, dy)
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, first, again):
        assert torch.equal(a, b), name
    assert EdgeConvBN is not None


@pytest.mark.parametrize("N,K,code", [(1025, 10, -3), (100, 65, -4), (100, 0, -4), (10, 11, -4)])
def test_beyond_limits_is_a_clean_error(N, K, code):
    from sg_pr_amd import engine
    from sg_pr_amd.train import EdgeConvBN
    P = torch.randn(1, 4, N, device="cuda")
    idx = torch.zeros(1, N, max(K, 1) if K > 0 else 0, dtype=torch.int64, device="cuda")
    with pytest.raises(engine.SgprError) as e:
        EdgeConvBN.apply(P, P.clone(), idx, torch.ones(4, device="cuda"), torch.zeros(4, device="cuda"), 1e-5)
    assert e.value.code == code
