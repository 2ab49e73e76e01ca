"""The stand-alone module entry points' argument checks (include/sgpr.h: sgpr_knn, sgpr_graph_feature,
sgpr_attention_pool(_any), sgpr_ntn(_any)), which all run before the device is touched.  CPU only: an empty batch is a
valid call with NULL data pointers, and every size outside the promised range keeps its error code, pointers or not."""
import ctypes

import pytest

SGPR_OK, SGPR_E_INVALID, SGPR_E_DIMS, SGPR_E_NODES, SGPR_E_K = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from sg_pr_amd import engine
    return engine.load_library()


@pytest.fixture(scope="module")
def ptr():
    """A non-NULL pointer the size checks must reject before any use of it (never dereferenced: no launch happens)."""
    buf = ctypes.create_string_buffer(64)
    return ctypes.cast(buf, ctypes.c_void_p), buf


def _calls(lib, p, B=0, C=3, N=10, k=5, F=32, T=16):
    return {
        "knn": lambda: lib.sgpr_knn(p, B, C, N, k, p, None),
        "graph_feature": lambda: lib.sgpr_graph_feature(p, p, B, C, N, k, p, None),
        "attention_pool": lambda: lib.sgpr_attention_pool(p, p, B, N, p, p, None),
        "attention_pool_any": lambda: lib.sgpr_attention_pool_any(p, p, B, N, F, p, p, None),
        "ntn": lambda: lib.sgpr_ntn(p, p, p, p, p, B, p, None),
        "ntn_any": lambda: lib.sgpr_ntn_any(p, p, p, p, p, B, F, T, p, None),
    }


@pytest.mark.parametrize("N,k,F,T", [(10, 5, 32, 16), (1, 1, 1, 1), (256, 32, 31, 15), (1024, 64, 128, 64), (300, 40, 33, 17)])
def test_empty_batch_with_null_pointers_is_ok(lib, N, k, F, T):
    for name, call in _calls(lib, None, B=0, C=128, N=N, k=k, F=F, T=T).items():
        assert call() == SGPR_OK, (name, lib.sgpr_last_error())


def test_null_pointers_with_a_batch_are_refused(lib):
    for name, call in _calls(lib, None, B=1).items():
        assert call() == SGPR_E_INVALID, name


@pytest.mark.parametrize("with_ptr", [False, True])
def test_sizes_out_of_range_keep_their_codes(lib, ptr, with_ptr):
    p = ptr[0] if with_ptr else None
    for B in (0, 1):
        # a negative batch
        for name, call in _calls(lib, p, B=-1).items():
            assert call() == SGPR_E_INVALID, name
        # sgpr_knn: channels, nodes, neighbours
        assert lib.sgpr_knn(p, B, 0, 10, 5, p, None) == SGPR_E_INVALID
        for N in (0, -3, 1025):
            assert lib.sgpr_knn(p, B, 3, N, 1, p, None) == SGPR_E_NODES, N
        for N, k in ((10, 0), (10, 11), (100, 65), (1024, 65), (5, -1)):
            assert lib.sgpr_knn(p, B, 3, N, k, p, None) == SGPR_E_K, (N, k)
        # sgpr_graph_feature: every size positive
        for C, N, k in ((0, 10, 5), (3, 0, 5), (3, 10, 0), (-1, 10, 5)):
            assert lib.sgpr_graph_feature(p, p, B, C, N, k, p, None) == SGPR_E_INVALID, (C, N, k)
        # attention: nodes, the tuned kernel's 12 288-node limit, the any-width kernel's widths
        assert lib.sgpr_attention_pool(p, p, B, 0, p, p, None) == SGPR_E_INVALID
        assert lib.sgpr_attention_pool(p, p, B, 12289, p, p, None) == SGPR_E_NODES
        assert lib.sgpr_attention_pool_any(p, p, B, 0, 32, p, p, None) == SGPR_E_INVALID
        for F in (0, -1, 129):
            assert lib.sgpr_attention_pool_any(p, p, B, 10, F, p, p, None) == SGPR_E_DIMS, F
        # the any-width NTN: widths and neurons
        for F, T in ((0, 16), (129, 16), (32, 0), (32, 65), (-1, -1)):
            assert lib.sgpr_ntn_any(p, p, p, p, p, B, F, T, p, None) == SGPR_E_DIMS, (F, T)
