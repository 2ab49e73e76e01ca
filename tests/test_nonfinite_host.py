"""The rule of tests/nonfinite_ref.py on the planted inputs of tests/test_gpu_score_nonfinite.py, without a GPU: which
pairs must be NaN, which are bound one-sidedly, that the float64 reference itself keeps every NaN, and that the checker
flags a kernel that swallows one (the fmaxf ReLU's sigmoid(fc2 . relu(fc1_b) + fc2_b))."""
import numpy as np
import pytest

import nonfinite_ref as nf
import score_ref


def _inputs(seed, r=37, m=131, f=32, scale=4.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, scale, size=(r, f)).astype(np.float32), rng.normal(0, scale, size=(m, f)).astype(np.float32))


def _any_shape_sd():
    from test_score_ref import _any_shape_sd as make
    return make()


@pytest.fixture(scope="module", params=["tuned", "any-shape"])
def case(request, oracle_sd):
    if request.param == "tuned":
        return oracle_sd, _inputs(7)
    return _any_shape_sd(), _inputs(7, f=48, scale=1.0)


def test_plant_bits_keeps_the_bits():
    a = np.zeros((3, 4), dtype=np.float32)
    nf.plant_bits(a, (1, slice(None)), nf.QNAN_NEG)
    nf.plant_bits(a, (2, 3), nf.QNAN_POS)
    assert (a.view(np.uint32)[1] == 0xFFC00000).all() and a.view(np.uint32)[2, 3] == 0x7FC00000
    assert np.isnan(a[1]).all() and np.isnan(a[2, 3]) and np.isfinite(a[0]).all() and np.isfinite(a[2, :3]).all()
    assert nf.element_indices(32) == [0, 15, 16, 31] and nf.element_indices(48) == [0, 23, 24, 47]


def test_classes_of_every_plant(case):
    sd, (rows, cols) = case
    clean_cls, clean = nf.classes(sd, rows, cols)
    assert (clean_cls == nf.FINITE).all() and np.isfinite(clean["score"]).all()
    names = set()
    for name, a, b, square in nf.plants(rows, cols):
        names.add(name)
        assert (b is a) == square
        cls, ref = nf.classes(sd, a, b)
        rbad, cbad = ~np.isfinite(a).all(axis=1), ~np.isfinite(b).all(axis=1)
        touched = rbad[:, None] | cbad[None, :]
        assert touched.any() and not touched.all(), name
        # exactly the pairs of a planted graph leave the FINITE class, counted from the plant
        assert ((cls != nf.FINITE) == touched).all(), name
        n_r, n_c = int(rbad.sum()), int(cbad.sum())
        assert int(touched.sum()) == n_r * b.shape[0] + n_c * a.shape[0] - n_r * n_c, name
        if "NaN" in name:
            assert (cls[touched] == nf.MUST_NAN).all() and np.isnan(ref["score"][touched]).all(), name
        else:
            assert np.isin(cls[touched], (nf.INF_BOUND, nf.INF_FREE)).all(), name
            assert ((cls == nf.INF_FREE) == (touched & np.isnan(ref["score"]))).all(), name
        # a pair of two healthy graphs does not depend on the planted ones
        if not square:
            assert np.array_equal(ref["score"][~touched], clean["score"][~touched]), name
        assert np.isfinite(ref["score"][~touched]).all(), name
    assert len(names) == 9
    # the last row and the last column are among the single-element plants
    by = {n: (a, b) for n, a, b, _ in nf.plants(rows, cols)}
    assert np.isnan(by["one NaN element in four rows"][0][-1]).sum() == 1
    assert np.isnan(by["one NaN element in four columns"][1][-1]).sum() == 1
    assert np.isinf(by["one +inf element in a row"][0][-1]).sum() == 1
    assert np.isinf(by["one -inf element in a column"][1][-1]).sum() == 1


def test_a_nan_with_an_infinity_is_a_nan(case):
    sd, (rows, cols) = case
    a = rows.copy()
    a[3, 0] = np.inf
    nf.plant_bits(a, (3, 5), nf.QNAN_POS)
    cls, ref = nf.classes(sd, a, cols)
    assert (cls[3] == nf.MUST_NAN).all() and (np.delete(cls, 3, axis=0) == nf.FINITE).all()


def test_the_checker_flags_a_swallowed_nan(case):
    sd, (rows, cols) = case
    p = score_ref.tail_weights(sd)
    swallowed = 1.0 / (1.0 + np.exp(-(np.maximum(p["fc1_b"], 0.0) @ p["fc2_w"] + p["fc2_b"])))   # fmaxf(NaN, 0) = 0
    assert 0.0 < swallowed < 1.0
    tol = np.full((rows.shape[0], cols.shape[0]), 3e-6)
    for name, a, b, _ in nf.plants(rows, cols):
        cls, ref = nf.classes(sd, a, b)
        t = tol[:a.shape[0], :b.shape[0]]
        exact = ref["score"].astype(np.float32)
        assert not nf.violations(exact, cls, ref, t).any(), name
        got = np.where(np.isnan(exact), np.float32(swallowed), exact)
        bad = nf.violations(got, cls, ref, t)
        assert (bad == (cls == nf.MUST_NAN)).all(), name           # INF_FREE owes nothing, MUST_NAN owes the NaN
        # one-sided: a NaN where the reference is not NaN passes for an infinite input, never for a finite one
        allnan = np.full(cls.shape, np.nan, dtype=np.float32)
        assert (nf.violations(allnan, cls, ref, t) == (cls == nf.FINITE)).all(), name
        off = np.where(np.isnan(exact), exact, exact + np.float32(1e-3))
        assert (nf.violations(off, cls, ref, t) == np.isin(cls, (nf.FINITE, nf.INF_BOUND))).all(), name
