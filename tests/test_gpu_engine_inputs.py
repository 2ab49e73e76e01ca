"""How Engine takes a resident score matrix and the optional outputs of the filters: every method that reads a matrix
gives the same bits whatever form the same values arrive in (a contiguous float32 device tensor, a row-strided view, a
column-strided view, a transposed-storage view, a float64 device tensor, a host array), row-strided out= / out_dir=
views receive the bits of the allocated outputs, and the wrapper refuses outputs and row_self tables of the wrong kind
with a ValueError before the library is called.

Before the binding took every resident matrix through one helper, each group of methods coerced it by a rule of its
own, and 9 of the 39 (method, shape) cases below did not hold on views whose strides do not matter or were not looked
at: the four filters read a column-strided [1, 7] view as if it were contiguous (wrong values: a one-row matrix was
never converted); topk_rows (k = 4), pair_positives, pair_threshold_counts and f1_max passed the raw row stride of a
one-row view, so a [1, 7] view with strides (1, 1) was refused by the library (SgprError, "leading dimension below M");
topk_rows (k = 4) asserted a unit column stride on a [5, 1] view with strides (1, 5).  All 30 other cases, the output
views and the rejections gave the same results then as now."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = ((5, 7), (1, 7), (5, 1))
FORMS = ("row_strided", "col_strided", "transposed", "float64", "host")


@pytest.fixture(scope="module")
def eng(ckpt_path):
    from oracle import sgpr_oracle
    from sg_pr_amd import engine
    e = engine.Engine(sgpr_oracle.load_checkpoint(ckpt_path), device=0)
    yield e
    e.close()


def _matrix(r, m):
    """seeded scores in (0, 1): host float32 [r, m]"""
    return np.random.default_rng(1000 * r + m).random((r, m), dtype=np.float32)


def _form(host, form):
    """the values of host [r, m] as a device tensor (or host array) of the given form"""
    r, m = host.shape
    if form == "host":
        return host.copy()
    dev = torch.from_numpy(host).cuda()
    if form == "contiguous":
        return dev
    if form == "float64":
        return dev.to(torch.float64)
    if form == "row_strided":
        buf = torch.full((r, m + 3), -7.0, dtype=torch.float32, device="cuda")
        buf[:, :m] = dev
        view = buf[:, :m]
        assert view.stride() == (m + 3, 1)
    elif form == "col_strided":
        buf = torch.full((r, 2 * m), -7.0, dtype=torch.float32, device="cuda")
        buf[:, ::2] = dev
        view = buf[:, ::2]
        assert view.stride(1) == 2
    else:
        assert form == "transposed"
        view = torch.as_strided(dev.t().contiguous(), (r, m), (1, r))
    assert view.shape == (r, m) and torch.equal(view, dev)
    return view


def _labels(r, m):
    """explicit ground truth int8 [r, m]: 1 / 0 / -1 (ignored)"""
    return np.random.default_rng(77 * r + m).integers(-1, 2, size=(r, m)).astype(np.int8)


def _poses(n, seed):
    return np.random.default_rng(seed).random((n, 2)) * 50.0


def _call(eng, method, score, host):
    from sg_pr_amd import engine
    r, m = host.shape
    thr = float(np.median(host))
    if method == "topk_rows":
        return eng.topk_rows(score, k=4)
    if method == "topk_rows_large":
        return eng.topk_rows_large(score, k=2)
    if method == "seq_filter":
        return eng.seq_filter(score, 2, want_dir=True)
    if method == "seq_path_filter":
        return eng.seq_path_filter(score, 2, engine.seq_paths(2, [1]), want_code=True)
    if method == "session_filter":
        return eng.session_filter(score, 2, want_code=True)
    if method == "peak_filter":
        return eng.peak_filter(score, 1)
    if method == "mine_rows":
        return eng.mine_rows(score, _poses(m, 5), k=2, row_pose=_poses(r, 6))
    if method == "rows_above":
        return eng.rows_above(score, thr)
    if method == "seq_rows_above":
        return eng.seq_rows_above(score, 2, thr)
    if method == "session_rows_above":
        return eng.session_rows_above(score, 2, thr)
    if method == "pair_positives":
        vals, bad = eng.pair_positives(score, gt=_labels(r, m))
        return torch.sort(vals).values, bad                    # (the list is unordered)
    if method == "pair_threshold_counts":
        return eng.pair_threshold_counts(score, [thr], gt=_labels(r, m))
    assert method == "f1_max"
    return eng.f1_max(score, gt=_labels(r, m))


METHODS = ("topk_rows", "topk_rows_large", "seq_filter", "seq_path_filter", "session_filter", "peak_filter", "mine_rows",
           "rows_above", "seq_rows_above", "session_rows_above", "pair_positives", "pair_threshold_counts", "f1_max")


def _bits(result):
    """a method's result as a list of (dtype, shape, bytes)"""
    out = []
    for x in result if isinstance(result, tuple) else (result,):
        if isinstance(x, torch.Tensor):
            x = x.cpu().numpy()
        x = np.ascontiguousarray(x) if x is not None else np.zeros(0, dtype=np.uint8)
        out.append((str(x.dtype), x.shape, x.tobytes()))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("method", METHODS)
def test_same_bits_whatever_form_the_matrix_arrives_in(eng, method, shape):
    host = _matrix(*shape)
    want = _bits(_call(eng, method, _form(host, "contiguous"), host))
    for form in FORMS:
        got = _bits(_call(eng, method, _form(host, form), host))
        assert got == want, (method, shape, form)


def _filter(eng, method, score, **kw):
    from sg_pr_amd import engine
    if method == "seq_filter":
        return eng.seq_filter(score, 2, **kw)
    if method == "seq_path_filter":
        return eng.seq_path_filter(score, 2, engine.seq_paths(2, [1]), **kw)
    if method == "session_filter":
        return eng.session_filter(score, 2, **kw)
    return eng.peak_filter(score, 1, **kw)


FILTERS = (("seq_filter", "out_dir"), ("seq_path_filter", "out_code"), ("session_filter", "out_code"), ("peak_filter", None))


def _strided(r, m, dtype, pad=3):
    buf = torch.zeros(r, m + pad, dtype=dtype, device="cuda")
    return buf[:, :m]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("method,second", FILTERS)
def test_row_strided_outputs_receive_the_allocated_bits(eng, method, second, shape):
    r, m = shape
    score = _form(_matrix(r, m), "contiguous")
    want_kw = {} if second is None else {"want_" + second[4:]: True}
    want = _bits(_filter(eng, method, score, **want_kw))
    outs = {"out": _strided(r, m, torch.float32)}
    if second is not None:
        outs[second] = _strided(r, m, torch.uint8)
    got = _filter(eng, method, score, **outs)
    for g, o in zip(got if isinstance(got, tuple) else (got,), outs.values()):
        assert g is o
    assert _bits(got) == want


@pytest.mark.parametrize("method,second", FILTERS)
def test_filters_refuse_outputs_of_the_wrong_kind(eng, method, second):
    r, m = 5, 7
    score = _form(_matrix(r, m), "contiguous")
    with pytest.raises(ValueError):
        _filter(eng, method, score, out=torch.empty(r, m + 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        _filter(eng, method, score, out=torch.empty(r, m, dtype=torch.float64, device="cuda"))
    if second is None:
        return
    with pytest.raises(ValueError):
        _filter(eng, method, score, **{second: torch.empty(r + 1, m, dtype=torch.uint8, device="cuda")})
    with pytest.raises(ValueError):
        _filter(eng, method, score, **{second: torch.empty(r, m, dtype=torch.int32, device="cuda")})
    with pytest.raises(ValueError):                                    # two outputs, two row strides
        _filter(eng, method, score, out=_strided(r, m, torch.float32, 3), **{second: _strided(r, m, torch.uint8, 5)})


def test_row_self_of_the_wrong_length_is_refused(eng):
    r, m = 5, 7
    host = _matrix(r, m)
    score = _form(host, "contiguous")
    thr = float(np.median(host))
    rs = torch.zeros(r + 1, dtype=torch.int32, device="cuda")
    pooled_rows, pooled_cols = torch.randn(r, eng.pw).cuda(), torch.randn(m, eng.pw).cuda()
    calls = (lambda: eng.topk_rows(score, k=4, row_self=rs),
             lambda: eng.topk_rows_large(score, k=2, row_self=rs),
             lambda: eng.session_filter(score, 2, row_self=rs),
             lambda: eng.peak_filter(score, 1, row_self=rs),
             lambda: eng.mine_rows(score, _poses(m, 5), k=2, row_self=rs),
             lambda: eng.rows_above(score, thr, row_self=rs),
             lambda: eng.seq_rows_above(score, 2, thr, row_self=rs),
             lambda: eng.session_rows_above(score, 2, thr, row_self=rs),
             lambda: eng.score_topk(pooled_rows, pooled_cols, k=1, row_self=rs),
             lambda: eng.score_topk(pooled_rows, pooled_cols, k=17, row_self=rs))
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d accepted a row_self of %d entries for %d rows" % (i, r + 1, r))
