"""The train-mode EdgeConv entry points' argument checks (include/sgpr.h: sgpr_edgeconv_train_forward / _backward,
sgpr_edgeconv_train_workspace_bytes), which all run before the device is touched.  CPU only: the pointers are NULL or a
host buffer that is never dereferenced, because every case returns before a launch."""
import ctypes

import pytest

SGPR_OK, SGPR_E_INVALID, SGPR_E_DIMS, SGPR_E_NODES, SGPR_E_K, SGPR_E_WORKSPACE = 0, -1, -2, -3, -4, -7
EPS = 1e-5


@pytest.fixture(scope="module")
def lib():
    from sg_pr_amd import engine
    return engine.load_library()


@pytest.fixture(scope="module")
def ptr():
    """A non-NULL pointer the checks must reject before any use of it (never dereferenced: no launch happens)."""
    buf = ctypes.create_string_buffer(64)
    return ctypes.cast(buf, ctypes.c_void_p), buf


def _forward(lib, ptrs, B, F, N, k, eps, ws):
    """ptrs: the 11 pointer arguments in the header's order (P Q idx gamma beta y sel s1 mean var workspace)."""
    p = list(ptrs)
    return lib.sgpr_edgeconv_train_forward(*p[:5], B, F, N, k, eps, *p[5:10], p[10], ws, None)


def _backward(lib, ptrs, B, F, N, k, eps, ws):
    """ptrs: the 15 pointer arguments (dy P Q idx sel s1 mean var gamma beta dP dQ dgamma dbeta workspace)."""
    p = list(ptrs)
    return lib.sgpr_edgeconv_train_backward(*p[:10], B, F, N, k, eps, *p[10:14], p[14], ws, None)


N_PTRS = {_forward: 11, _backward: 15}
ENTRIES = pytest.mark.parametrize("call", [_forward, _backward], ids=["forward", "backward"])


def _ws(lib, B, F):
    return int(lib.sgpr_edgeconv_train_workspace_bytes(B, F))


def test_workspace_bytes(lib):
    for B, F in ((1, 1), (16, 64), (70000, 1), (3, 1000003), (65535, 65535)):
        assert _ws(lib, B, F) == 16 * B * F, (B, F)
    for B, F in ((0, 1), (1, 0), (-1, 5), (5, -1), (0, 0), (-2 ** 31, 64)):
        assert _ws(lib, B, F) == 16, (B, F)


@ENTRIES
@pytest.mark.parametrize("with_ptr", [False, True])
def test_invalid_sizes(lib, ptr, call, with_ptr):
    ps = [ptr[0] if with_ptr else None] * N_PTRS[call]
    ws = 1 << 40
    for B, F, eps in ((0, 8, EPS), (-1, 8, EPS), (1, 0, EPS), (1, -8, EPS), (1, 8, -1e-5), (1, 8, float("nan")),
                      (1, 8, -float("inf"))):
        assert call(lib, ps, B, F, 100, 10, eps, ws) == SGPR_E_INVALID, (B, F, eps)
    assert call(lib, ps, 2, 8, 100, 10, 0.0, 0) == SGPR_E_WORKSPACE      # eps = 0 is valid
    for N in (0, -1, 1025, 4096):
        assert call(lib, ps, 1, 8, N, 1, EPS, ws) == SGPR_E_NODES, N
    for N, k in ((100, 0), (100, -1), (100, 65), (1024, 65), (10, 11), (1, 2), (64, 65)):
        assert call(lib, ps, 1, 8, N, k, EPS, ws) == SGPR_E_K, (N, k)


@ENTRIES
@pytest.mark.parametrize("B,F,N,k", [(1, 1, 1, 1), (16, 64, 100, 10), (2, 100, 1024, 64), (70000, 1, 4, 2),
                                     (3, 257, 37, 37)])
def test_workspace_one_byte_short(lib, ptr, call, B, F, N, k):
    for ps in ([None] * N_PTRS[call], [ptr[0]] * N_PTRS[call]):
        assert call(lib, ps, B, F, N, k, EPS, _ws(lib, B, F) - 1) == SGPR_E_WORKSPACE
        assert call(lib, ps, B, F, N, k, EPS, 0) == SGPR_E_WORKSPACE


@ENTRIES
def test_one_null_pointer(lib, ptr, call):
    B, F, N, k = 2, 8, 100, 10
    n = N_PTRS[call]
    for i in range(n):
        ps = [ptr[0]] * n
        ps[i] = None
        assert call(lib, ps, B, F, N, k, EPS, _ws(lib, B, F)) == SGPR_E_INVALID, i
    assert call(lib, [None] * n, B, F, N, k, EPS, _ws(lib, B, F)) == SGPR_E_INVALID


# (N, k, F): F passes a bound on the scatter kernel's channel tile (16 / 32 / 64 wide here) but needs more than 65 535
# tiles of the stats / grad kernels' narrower one (8 / 16 / 32 wide); then rows where the scatter tile is the narrower
# one or both are 64 wide, and an F whose tile count overflows 32-bit arithmetic
TOO_WIDE = [(1024, 1, 600000), (1024, 2, 600000), (512, 9, 1100000), (256, 22, 2200000), (256, 23, 2200000),
            (1024, 64, 2 * 65535 + 1), (100, 10, 65535 * 64 + 1), (1, 1, 2 ** 31 - 1), (1024, 1, 2 ** 31 - 1)]


@ENTRIES
@pytest.mark.parametrize("N,k,F", TOO_WIDE)
def test_too_many_channel_tiles(lib, ptr, call, N, k, F):
    for ps in ([None] * N_PTRS[call], [ptr[0]] * N_PTRS[call]):
        for ws in (0, 1 << 62):
            assert call(lib, ps, 1, F, N, k, EPS, ws) == SGPR_E_DIMS, ws
            assert "channel tiles" in lib.sgpr_last_error().decode()


# the channel tiles of csrc/sgpr_train.hip (pick_tile), for F >= 64: the widest power of two <= 64 whose LDS fits the
# stats / grad kernels' 56 KB budget (an fp32 row of N | 1 floats per channel) and the scatter kernel's 160 KB one (a
# fixed part for the reverse adjacency, then two fp32 rows and one byte row per channel)
def _tiles(N, k):
    row = N | 1
    fixed = ((2 * N + 1 + 2 * 256) * 4 + N * k * 2 + 15) & ~15
    stats = max(t for t in (1, 2, 4, 8, 16, 32, 64) if t * row * 4 <= 56 * 1024)
    scatter = max(t for t in (1, 2, 4, 8, 16, 32, 64) if fixed + t * (2 * row * 4 + N) <= 160 * 1024)
    return stats, scatter


def test_tile_model_matches_the_documented_rows():
    assert _tiles(1024, 1) == (8, 16) and _tiles(512, 9) == (16, 32) and _tiles(256, 22) == (32, 64)
    assert _tiles(256, 23) == (32, 32) and _tiles(100, 10) == (64, 64) and _tiles(1024, 64) == (8, 2)


@ENTRIES
def test_widest_launchable_F_over_the_whole_range(lib, call):
    """For every (N, k) of the promised range, the widest F that both kernels' tiles launch in <= 65 535 tiles reaches
    the next check (the workspace) and one channel more is SGPR_E_DIMS."""
    ps = [None] * N_PTRS[call]
    narrower_stats = 0
    for N in range(1, 1025):
        for k in range(1, min(N, 64) + 1):
            stats, scatter = _tiles(N, k)
            narrower_stats += stats < scatter
            F = 65535 * min(stats, scatter)
            assert call(lib, ps, 1, F, N, k, EPS, 0) == SGPR_E_WORKSPACE, (N, k, F)
            assert call(lib, ps, 1, F + 1, N, k, EPS, 0) == SGPR_E_DIMS, (N, k, F + 1)
    assert narrower_stats == 4144


def test_tie_exact_reference_agrees_with_the_dense_max():
    """train_ref.pq_block_selected on continuous inputs (no ties) is pq_block, values and gradients; on ties it picks
    the lowest k, on P (largest for gamma >= 0, smallest for gamma < 0), after clamping the list."""
    import torch
    from train_ref import pq_block, pq_block_selected
    g = torch.Generator().manual_seed(0)
    B, F, N, K = 3, 6, 20, 5
    idx = torch.randint(0, N, (B, N, K), generator=g)
    leaves = [torch.randn(B, F, N, generator=g, dtype=torch.float64), torch.randn(B, F, N, generator=g,
                                                                                   dtype=torch.float64),
              torch.tensor([1.0, -0.5, 0.7, -2.0, 1.5, -1.0], dtype=torch.float64),
              torch.randn(F, generator=g, dtype=torch.float64)]
    dy = torch.randn(B, F, N, generator=g, dtype=torch.float64)
    outs = []
    for fn in (pq_block, pq_block_selected):
        t = [v.clone().requires_grad_(True) for v in leaves]
        r = fn(t[0], t[1], idx, t[2], t[3])
        r[0].backward(dy)
        outs.append([v.detach() for v in r[:3]] + [v.grad for v in t])
    for a, b in zip(*outs):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)

    P = torch.tensor([[[3.0, 1.0, 3.0, 1.0]], [[3.0, 1.0, 3.0, 1.0]]], dtype=torch.float64)   # B = 2, F = 1, N = 4
    idx = torch.tensor([[[1, 0, 2, 3]] * 4, [[3, 1, 9, -7]] * 4])       # graph 1: 9 -> 3, -7 -> 0
    for gamma, want in ((1.0, [1, 3]), (0.0, [1, 3]), (-1.0, [0, 0])):
        _, _, _, sel, s1 = pq_block_selected(P, torch.zeros_like(P), idx, torch.tensor([gamma], dtype=torch.float64),
                                             torch.zeros(1, dtype=torch.float64))
        assert sel[0, 0].tolist() == [want[0]] * 4 and sel[1, 0].tolist() == [want[1]] * 4, gamma
        assert s1[0, 0].tolist() == [8.0] * 4 and s1[1, 0].tolist() == [6.0] * 4
