"""sgpr_session_rows_above / sgpr_score_session_above off the GPU: the symbols, the host-side argument checks, the workspace
identities, the NumPy reference (tests/session_above_ref.py) against session_ref / seq_above_ref and by hand, the planted
three-session world under a threshold, the place database's routing on a stub engine, and precision_recall_at with a
session table.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

import seq_above_ref
import seq_path_ref
import session_above_ref as sar
import session_ref
from test_seq_paths_host import _bad_tables, _random_scores, _table, _zeroed_handle
from test_session_host import _StubModel, _bad_session_tables, _starts, _vec

FWD, REV, CAUSAL = 2, 4, 1
MODES = [(True, False), (False, True), (True, True)]
INF = float("inf")
NEW = ("sgpr_session_rows_above_workspace_bytes", "sgpr_session_rows_above",
       "sgpr_score_session_above_workspace_bytes", "sgpr_score_session_above")


def test_symbols_present_and_abi_unchanged():
    from sg_pr_amd import engine
    lib = engine.load_library()
    assert lib.sgpr_abi_version() == 11
    for name in NEW:
        assert name in engine.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    for name in ("session_rows_above", "score_session_above", "session_rows_above_workspace_bytes",
                 "score_session_above_workspace_bytes"):
        assert callable(getattr(engine.Engine, name))


# ------------------------------------------------------------------------------------------------- argument checks
def _common_checks(lib, call, R, M, resident):
    """every argument error both calls share; `call` takes keyword overrides"""
    assert call(h=None) == -1
    assert call(count=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(cap=-1) == -1 and b"capacity" in lib.sgpr_last_error()
    for which in ("orows", "ocols", "ovals"):
        assert call(**{which: None}) == -1, which
    assert call(thr=float("nan")) == -1 and b"NaN" in lib.sgpr_last_error()
    assert call(window=-2) == -1 and b"window" in lib.sgpr_last_error()
    for L in (0, 33, -1):
        assert call(L=L, mt=1) == -1 and b"sequence length" in lib.sgpr_last_error()
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
    for flags in (0, CAUSAL):
        assert call(flags=flags) == -1 and b"direction" in lib.sgpr_last_error()
    assert call(flags=FWD | 8) == -1 and b"flag" in lib.sgpr_last_error()
    for n in (17, -1):
        assert call(n=n) == -1 and b"n_paths" in lib.sgpr_last_error()
    assert call(n=0) == -1 and b"n_paths = 0" in lib.sgpr_last_error()
    assert call(table=None) == -1 and b"NULL path table" in lib.sgpr_last_error()
    for bad, word in _bad_tables(8):
        t, tp = _table(bad)
        assert call(table=tp, n=t.shape[0]) == -1 and word in lib.sgpr_last_error(), (bad, lib.sgpr_last_error())
    for which, limit, word in (("r", R, b"row"), ("c", M, b"column")):
        for values, n, msg in _bad_session_tables(limit):
            t, tp = (None, None) if values is None else _starts(values)
            kw = {which + "starts": tp, "n" + which: len(values) if n is None else n}
            assert call(**kw) == -1, (which, values, n)
            assert msg in lib.sgpr_last_error() and word in lib.sgpr_last_error(), (values, n, lib.sgpr_last_error())
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    for mt in (0, 9, -1, 33):
        assert call(mt=mt) == -1 and b"min_terms" in lib.sgpr_last_error(), mt
    assert call(L=1, table=None, n=0, mt=2) == -1 and b"min_terms" in lib.sgpr_last_error()
    assert call(ws_bytes=call.need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7


def test_session_rows_above_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300
    good, good_p = _table(seq_path_ref.seq_paths(8, seq_path_ref.SLOPES))
    rt, rt_p = _starts([0, 40, 40, 100])
    ct, ct_p = _starts([0, 1, 300])
    wsb = lib.sgpr_session_rows_above_workspace_bytes
    need = wsb(h, R, M, 7)
    assert need > 0 and need == lib.sgpr_seq_rows_above_workspace_bytes(h, R, M, 7)

    def call(h=h, score=p, ld=M, ctx=7, row0=0, window=3, flags=FWD | REV, L=8, table=good_p, n=good.shape[0],
             rstarts=rt_p, nr=4, cstarts=ct_p, nc=3, mt=2, thr=0.5, orows=p, ocols=p, ovals=p, cap=10, count=p, ws=p,
             ws_bytes=need, r=R):
        return lib.sgpr_session_rows_above(h, score, r, M, ld, ctx, None, row0, window, flags, L, table, n, rstarts, nr,
                                           cstarts, nc, mt, thr, orows, ocols, ovals, None, cap, None, count, ws, ws_bytes,
                                           None)
    call.need = need
    _common_checks(lib, call, R, M, True)
    assert call(score=None) == -1 and b"NULL score" in lib.sgpr_last_error()
    assert call(ld=M - 1) == -1 and b"ld" in lib.sgpr_last_error()
    for bad in ((None, R, M, 7), (h, -1, M, 0), (h, R, -1, 7), (h, R, M, -1), (h, R, M, R + 1), (h, R, M, R), (h, R, 0, 7)):
        assert wsb(*bad) == 0, bad[1:]


def test_score_session_above_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)
    R, M = 100, 300
    good, good_p = _table(seq_path_ref.seq_paths(8, seq_path_ref.SLOPES))
    P = good.shape[0]
    rt, rt_p = _starts([0, 7, 40, 100])
    ct, ct_p = _starts([0, 150])
    wsb = lib.sgpr_score_session_above_workspace_bytes
    need = wsb(h, R, M, 7, 8, P, FWD | REV, 4, 2)
    assert need > 0

    def call(h=h, rows=p, cols=p, ctx=7, row0=0, window=10, flags=FWD | REV, L=8, table=good_p, n=P, rstarts=rt_p, nr=4,
             cstarts=ct_p, nc=2, mt=4, thr=0.5, orows=p, ocols=p, ovals=p, cap=10, count=p, ws=p, ws_bytes=need, r=R):
        return lib.sgpr_score_session_above(h, rows, r, cols, M, ctx, None, row0, window, flags, L, table, n, rstarts, nr,
                                            cstarts, nc, mt, thr, orows, ocols, ovals, None, cap, None, count, ws, ws_bytes,
                                            None)
    call.need = need
    _common_checks(lib, call, R, M, False)
    assert call(rows=None) == -1 and b"NULL pooled" in lib.sgpr_last_error()
    assert call(cols=None) == -1
    # the workspace answer is 0 for invalid arguments
    for L in (0, 33, -2):
        assert wsb(h, R, M, 7, L, P, FWD, 4, 2) == 0
    for ctx in (-1, R + 1):
        assert wsb(h, R, M, ctx, 8, P, FWD, 4, 2) == 0
    for flags in (0, CAUSAL, FWD | 8):
        assert wsb(h, R, M, 7, 8, P, flags, 4, 2) == 0
    for n in (17, -1):
        assert wsb(h, R, M, 7, 8, n, FWD, 4, 2) == 0
    for n in (-1, 65):
        assert wsb(h, R, M, 7, 8, P, FWD, n, 2) == 0 and wsb(h, R, M, 7, 8, P, FWD, 4, n) == 0
    assert wsb(None, R, M, 7, 8, P, FWD, 4, 2) == 0 and wsb(h, -1, M, 0, 8, P, FWD, 4, 2) == 0
    assert wsb(h, R, M, R, 8, P, FWD, 4, 2) == 0 and wsb(h, R, 0, 7, 8, P, FWD, 4, 2) == 0      # empty: nothing needed


def test_workspace_identities():
    """the pooled workspace is sgpr_score_seq_above's at equal R, M, ctx, L, flags, whatever the paths and tables hold"""
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    wsb, seq = lib.sgpr_score_session_above_workspace_bytes, lib.sgpr_score_seq_above_workspace_bytes
    for R, M in ((100, 300), (300, 517), (20000, 20000), (150, 262144)):
        for L in (1, 8, 32):
            ctx = min(L - 1, R)
            for flags in (FWD, REV | CAUSAL, FWD | REV, FWD | REV | CAUSAL):
                want = seq(h, R, M, ctx, L, flags)
                assert want > 0
                for n in (0, 1, 9, 16):
                    for nr, nc in ((0, 0), (1, 1), (4, 64), (64, 3)):
                        assert wsb(h, R, M, ctx, L, n, flags, nr, nc) == want
            assert lib.sgpr_session_rows_above_workspace_bytes(h, R, M, ctx) == \
                lib.sgpr_seq_rows_above_workspace_bytes(h, R, M, ctx) > 0
    assert 0 < wsb(h, 300000, 300000, 31, 32, 16, FWD, 64, 64) < 1e9     # never R x M


# ------------------------------------------------------------------------------------------------- the reference itself
def _bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _same(got, want, what):
    assert len(got) == len(want) == 5
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            _bits(g, w, (what, j))
        else:
            assert np.array_equal(g, w), (what, j)


TABLES = [(40, 70, [0, 1, 2, 17, 17, 39], [0, 1, 33, 34, 34, 34, 69, 70]), (33, 50, [0, 0, 5, 33], [0, 0, 0, 25, 50, 50]),
          (20, 300, None, [0, 255, 256, 257]), (37, 45, [0, 20], None)]


@pytest.mark.parametrize("case", TABLES, ids=["%dx%d" % c[:2] for c in TABLES])
def test_reference_min_terms_one_is_the_session_filter(case):
    """min_terms = 1: session_ref.session_filter's Q and code, then seq_above_ref.select under the session window"""
    r, m, rt, ct = case
    s = _random_scores(r, m, 5 * r + m)
    rng = np.random.default_rng(r)
    explicit = rng.integers(-2, m + 3, size=r).astype(np.int32)
    n = 0
    for L in (1, 2, 8, 32):
        for name, paths in (("unit", None), ("nine", seq_path_ref.seq_paths(L, seq_path_ref.SLOPES))):
            for fwd, rev in MODES:
                for ctx in sorted({0, min(L - 1, r), r}):
                    kw = dict(ctx=ctx, forward=fwd, reverse=rev, row_starts=rt, col_starts=ct)
                    q, code, have = sar.fold(s, paths, L, min_terms=1, **kw)
                    wq, wc = session_ref.session_filter(s, paths, L=L, **kw)
                    assert have.all()
                    what = (case, L, name, fwd, rev, ctx)
                    assert np.array_equal(q.view(np.uint32), wq.view(np.uint32)), what      # NaN payloads included
                    assert np.array_equal(code, wc), what
                    window = (-1, 0, 3)[n % 3]
                    who = (dict(row0=0), dict(row0=7), dict(row_self=explicit))[n % 3]
                    causal = bool(n % 2)
                    n += 1
                    ok = np.ones((r - ctx, m), dtype=bool)
                    if window >= 0:
                        ok &= ~session_ref.excluded(r, m, ct, window, who.get("row_self"), who.get("row0", 0))[ctx:]
                    if causal:
                        ok &= seq_above_ref.eligible(r, m, ctx, -1, who.get("row0", 0), True, who.get("row_self"))
                    for thr in (-INF, 0.5, INF):
                        got = sar.session_above(s, thr, paths, L, min_terms=1, window=window, causal=causal, **who, **kw)
                        _same(got, seq_above_ref.select(wq, wc, ok, thr), what + (window, causal, thr))


@pytest.mark.parametrize("L", [1, 2, 8, 32])
def test_reference_one_session_unit_path_is_seq_above(L):
    for r, m in ((1, 1), (5, 7), (40, 70), (70, 33)):
        s = _random_scores(r, m, 13 * r + m)
        n = 0
        for fwd, rev in MODES:
            for ctx in sorted({0, min(L - 1, r), r}):
                for thr in (-INF, 0.5, 0.75):
                    elig = (dict(window=-1), dict(window=3, row0=2), dict(window=0, causal=True),
                            dict(window=5, causal=True, row_self=np.arange(r, dtype=np.int32)[::-1] % m))[n % 4]
                    n += 1
                    want = seq_above_ref.seq_above(s, L, thr, ctx=ctx, forward=fwd, reverse=rev, **elig)
                    for tables in (dict(), dict(row_starts=[0], col_starts=[0])):
                        got = sar.session_above(s, thr, None, L, ctx=ctx, forward=fwd, reverse=rev, min_terms=1, **tables,
                                                **elig)
                        _same(got, want, (L, r, m, fwd, rev, ctx, thr, sorted(elig)))


def _listed(result, r, c):
    rows, cols = result[0], result[1]
    hit = np.flatnonzero((rows == r) & (cols == c))
    return None if hit.size == 0 else (result[2][hit[0]], int(result[3][hit[0]]))


def test_rule_rows_after_a_session_start():
    """a row j rows after a session start has j + 1 terms: eligible at min_terms = j + 1 and not at j + 2"""
    L, r, m = 8, 30, 40
    s = _random_scores(r, m, 3)
    s = np.where(np.isfinite(s), s, np.float32(0.25)).astype(np.float32)
    for start in (0, 11):
        rt = [0, start] if start else None
        for j in range(L):
            row = start + j
            for mt in range(1, L + 1):
                got = sar.session_above(s, -INF, None, L, forward=True, row_starts=rt, min_terms=mt)
                listed = int(np.sum(got[0] == row))
                if mt <= j + 1:
                    assert listed == (m - (mt - 1)), (start, j, mt, listed)      # columns c >= mt - 1 reach mt terms
                else:
                    assert listed == 0, (start, j, mt, listed)
                assert got[4][-1] == got[0].size
    # a row past the first L - 1 of its session is limited by its column alone
    got = sar.session_above(s, -INF, None, L, forward=True, row_starts=[0, 11], min_terms=L)
    assert int(np.sum(got[0] == 11 + L - 1)) == m - (L - 1) and int(np.sum(got[0] == 11 + L - 2)) == 0


def test_rule_short_forward_full_reverse_takes_the_reverse():
    """beside a column seam the forward candidate is short and the reverse candidate is full: the reverse value and code
    are taken, even where the short forward mean is larger"""
    L, r, m = 4, 6, 12
    s = np.full((r, m), 0.125, dtype=np.float32)
    ct = [0, 5]                                        # column 5 starts a session: forward from (5, 5) has one term
    s[5, 5] = 0.875                                    # ... whose mean is the entry itself
    fwd_q, fwd_n = sar.candidate(s, np.arange(L), +1, np.zeros(r, np.int64), session_ref.lo(ct, np.arange(m)),
                                 session_ref.hi(ct, np.arange(m), m))
    rev_q, rev_n = sar.candidate(s, np.arange(L), -1, np.zeros(r, np.int64), session_ref.lo(ct, np.arange(m)),
                                 session_ref.hi(ct, np.arange(m), m))
    assert fwd_n[5, 5] == 1 and rev_n[5, 5] == 4 and fwd_q[5, 5] > rev_q[5, 5]
    one = sar.session_above(s, -INF, None, L, forward=True, reverse=True, col_starts=ct, min_terms=1)
    v, code = _listed(one, 5, 5)
    assert v == np.float32(0.875) and code == 0        # today's prefix rule: the one-term forward mean wins
    two = sar.session_above(s, -INF, None, L, forward=True, reverse=True, col_starts=ct, min_terms=2)
    v, code = _listed(two, 5, 5)
    assert v == rev_q[5, 5] == np.float32((0.875 + 3 * 0.125)) * session_ref.RCP[4] and code == 1
    # forward alone: the end point is not eligible, not even at -inf
    assert _listed(sar.session_above(s, -INF, None, L, forward=True, col_starts=ct, min_terms=2), 5, 5) is None
    # with a path table the code names the path: the all-zero path has L terms everywhere below row L - 1
    paths = np.array([[0, 1, 2, 3], [0, 0, 0, 0]], dtype=np.int32)
    got = sar.session_above(s, -INF, paths, forward=True, reverse=False, col_starts=ct, min_terms=4)
    v, code = _listed(got, 5, 5)
    assert code == 2 and v == np.float32((0.875 + 3 * 0.125)) * session_ref.RCP[4]


def test_rule_nan_terms():
    L, r, m = 4, 8, 16
    base = np.full((r, m), 0.5, dtype=np.float32)
    ct = [0, 8]
    # a NaN among the terms of a participating candidate: NaN out, never listed
    s = base.copy()
    s[5, 3] = np.nan                                   # a term of forward (7, 5): rows 7, 6, 5 <-> columns 5, 4, 3
    got = sar.session_above(s, -INF, None, L, forward=True, col_starts=ct, min_terms=3)
    q, code, have = sar.fold(s, None, L, forward=True, col_starts=ct, min_terms=3)
    assert have[7, 5] and np.isnan(q[7, 5]) and _listed(got, 7, 5) is None
    assert _listed(got, 7, 6) is not None
    # ... in both directions the other candidate replaces a NaN best (the fold's rule)
    got = sar.session_above(s, -INF, None, L, forward=True, reverse=True, col_starts=ct, min_terms=3)
    assert _listed(got, 7, 5) == (np.float32(0.5), 1)
    # a NaN only in a candidate that does not participate changes nothing
    s = base.copy()
    s[6, 9] = np.nan                                   # forward (7, 10): columns 10, 9, 8 - three terms, below min_terms 4
    s[7, 10] = 0.75
    clean = base.copy()
    clean[7, 10] = 0.75
    a = sar.session_above(s, -INF, None, L, forward=True, reverse=True, col_starts=ct, min_terms=4)
    b = sar.session_above(clean, -INF, None, L, forward=True, reverse=True, col_starts=ct, min_terms=4)
    assert _listed(a, 7, 10) == _listed(b, 7, 10) == (np.float32(0.75 + 3 * 0.5) * session_ref.RCP[4], 1)
    # ... forward alone at min_terms = 3: that candidate participates, and the end point is NaN and never listed
    assert _listed(sar.session_above(s, -INF, None, L, forward=True, col_starts=ct, min_terms=3), 7, 10) is None
    assert _listed(sar.session_above(clean, -INF, None, L, forward=True, col_starts=ct, min_terms=3), 7, 10) == \
        (np.float32(0.75 + 2 * 0.5) * session_ref.RCP[3], 0)


def test_rule_minus_inf_lists_every_eligible_pair_and_no_other():
    r, m, L = 33, 50, 8
    s = _random_scores(r, m, 17)
    rt, ct = [0, 0, 5, 33], [0, 0, 0, 25, 50, 50]
    for mt in (1, 2, 5, 8):
        for fwd, rev in MODES:
            for kw in (dict(window=-1), dict(window=4, row0=20), dict(window=4, row0=20, causal=True)):
                q, code, have = sar.fold(s, None, L, ctx=3, forward=fwd, reverse=rev, row_starts=rt, col_starts=ct,
                                         min_terms=mt)
                ok = sar.eligible(r, m, 3, have, ct, kw["window"], kw.get("row0", 0), kw.get("causal", False))
                got = sar.session_above(s, -INF, None, L, ctx=3, forward=fwd, reverse=rev, row_starts=rt, col_starts=ct,
                                        min_terms=mt, **kw)
                mask = np.zeros((r - 3, m), dtype=bool)
                mask[got[0], got[1]] = True
                assert np.array_equal(mask, ok & ~np.isnan(q)), (mt, fwd, rev, kw)
                assert not mask[~have].any() and (mt == 1 or not have.all())
                assert np.array_equal(got[4], np.concatenate(([0], np.cumsum(mask.sum(axis=1)))))


# ------------------------------------------------------------------------------------------------- the planted world
def planted_row(seed, L, min_terms, threshold=0.7, window=50):
    """(accepted pairs, precision, recall of the 300 planted pairs, B-head rows 150..174 found) of the session form"""
    s, col = session_ref.planted(seed)
    got = sar.session_above(s, threshold, None, L, forward=True, reverse=True, row_starts=session_ref.WORLD_STARTS,
                            col_starts=session_ref.WORLD_STARTS, min_terms=min_terms, window=window)
    n, precision, recall = sar.precision_recall(got[0], got[1], col)
    head = (got[0] >= 150) & (got[0] < 175) & (col[got[0]] == got[1])
    return n, precision, recall, int(head.sum()), got


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_planted_sessions_under_a_threshold(seed):
    """L = 8, both directions, session window 50, threshold 0.7.  Measured over seeds 0..4 (min - max):
    min_terms 1: 913 - 1011 pairs, precision 0.297 - 0.329, recall 0.990 - 1.000, B head 25 of 25;
    min_terms 2: 483 - 532, 0.560 - 0.617, 0.983 - 0.993, 24;  min_terms 4: 310 - 321, 0.916 - 0.945, 0.970 - 0.980, 22;
    min_terms 8: 286 - 296, 0.966 - 0.990, 0.943 - 0.953, 18.  Each gate lies 0.05 inside the observed extreme."""
    one = planted_row(seed, 8, 1)
    four = planted_row(seed, 8, 4)
    print("seed", seed, "min_terms 1 (pairs, precision, recall, B head):", one[:4], "min_terms 4:", four[:4])
    assert one[1] <= 0.38                              # the prefix rule: one- and two-term means are noise above T
    assert four[1] >= 0.86
    assert four[2] >= 0.92
    # the one-trajectory form finds none of the B-head rows: the partner 299 - r lies within 50 indices
    s, col = session_ref.planted(seed)
    flat = seq_above_ref.seq_above(s, 8, 0.7, forward=True, reverse=True, window=50)
    assert int(np.sum((flat[0] >= 150) & (flat[0] < 175) & (col[flat[0]] == flat[1]))) == 0
    # the session form at min_terms = 4: rows 150..152 have fewer than 4 terms and are never listed; measured 22 of the
    # other 22 on every seed, gated one row in twenty below (0.05 of 22, rounded up: 2 rows)
    assert not np.isin(four[4][0], (150, 151, 152)).any()
    assert 20 <= four[3] <= 22


# ------------------------------------------------------------------------------------------------- the place database
class _AboveStub:
    """the engine calls the closure queries make, recorded; vectors stay on the CPU"""
    pw = 8
    device = torch.device("cpu")

    class dims:
        pass

    def __init__(self):
        self.calls = []

    def _pooled(self, t, name):
        return torch.as_tensor(t, dtype=torch.float32).reshape(-1, self.pw)

    def score_session_above(self, rows, cols, L, threshold, paths=None, **kw):
        self.calls.append(("score_session_above", tuple(rows.shape), tuple(cols.shape), (L, threshold, paths), kw))
        n = rows.shape[0] - kw.get("context", 0)
        e = torch.zeros(0, dtype=torch.int32)
        return e, e, torch.zeros(0), torch.zeros(0, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.int64)


@pytest.fixture
def above_db(monkeypatch):
    from sg_pr_amd import place_db
    for f in place_db._DIMS:
        setattr(_AboveStub.dims, f, 1)
    monkeypatch.setattr(place_db, "weights_sha256", lambda model: "stub")
    model = _StubModel()
    model._eng = _AboveStub()
    return place_db.PlaceDatabase(model, capacity=2), model


def test_place_database_closure_routing(above_db):
    db, model = above_db
    calls = model.engine().calls
    db.append_pooled(_vec(5))
    # one session: the session call all the same
    out = db.query_closures(None, None, 0.5, seq_len=4, min_terms=2, window=3, causal=True, pooled=_vec(1))
    name, rows, cols, a, kw = calls[-1]
    assert len(out) == 5 and name == "score_session_above" and rows == (4, 8) and cols == (5, 8)
    assert a == (4, 0.5, None) and kw["context"] == 3 and kw["row0"] == 2 and kw["min_terms"] == 2 and kw["causal"]
    assert kw["col_sessions"].tolist() == [0] and kw.get("row_sessions") is None and kw["window"] == 3
    assert kw["reverse"] == "both"
    db.query_ids_closures(1, 3, 0.25, seq_len=4, slopes=["1", "2"], window=3, reverse=True)
    name, rows, cols, a, kw = calls[-1]
    assert rows == (4, 8) and a[0] == 4 and a[1] == 0.25 and a[2].shape == (2, 4) and kw["context"] == 1
    assert kw["row0"] == 0 and kw["row_sessions"].tolist() == [0] and kw["col_sessions"].tolist() == [0]
    assert kw["min_terms"] == 1 and kw["reverse"] is True and not kw["causal"]
    db.query_closures(None, None, 0.5, pooled=_vec(2))                     # seq_len = 1: no context rows
    assert calls[-1][1] == (2, 8) and calls[-1][3][0] == 1 and calls[-1][4]["context"] == 0 and calls[-1][4]["row0"] == 5
    # three sessions
    db.new_session()
    out = db.query_closures(None, None, 0.5, seq_len=4, min_terms=4, window=3, causal=True, pooled=_vec(1))
    name, rows, cols, a, kw = calls[-1]
    assert rows == (1, 8) and kw["context"] == 0 and kw["row0"] == 5 and kw["col_sessions"].tolist() == [0, 5]
    db.append_pooled(_vec(2, 1))
    db.query_closures(None, None, 0.5, seq_len=4, pooled=_vec(2), slopes=["1", "1/2"])
    name, rows, cols, a, kw = calls[-1]
    assert rows == (4, 8) and cols == (7, 8) and kw["context"] == 2 and kw["row0"] == 5      # members of the current session
    assert a[2].shape == (3, 4)
    db.append_pooled(_vec(6, 2))
    db.new_session()
    db.append_pooled(_vec(1, 3))
    assert db.session_starts.tolist() == [0, 5, 13] and len(db) == 14
    db.query_ids_closures(6, 8, 0.5, seq_len=4, min_terms=3, window=2, reverse=True)
    name, rows, cols, a, kw = calls[-1]
    assert rows == (11, 8) and cols == (14, 8) and kw["context"] == 3 and kw["row0"] == 3 and kw["min_terms"] == 3
    assert kw["row_sessions"].tolist() == [0, 2, 10] and kw["col_sessions"].tolist() == [0, 5, 13]
    db.query_ids_closures(0, 14, 0.5)
    assert calls[-1][4]["row_sessions"].tolist() == [0, 5, 13] and calls[-1][3][0] == 1
    with pytest.raises(IndexError):
        db.query_ids_closures(10, 5, 0.5)
    assert all(c[0] == "score_session_above" for c in calls)
    # the four thresholded queries of one trajectory still raise, and point to the new ones
    for bad in (lambda: db.query_ids_above([0], 0.5), lambda: db.query_above(None, None, 0.5),
                lambda: db.query_seq_above(None, None, 4, 0.5, pooled=_vec(1)),
                lambda: db.query_ids_seq_above(0, 3, 4, 0.5)):
        with pytest.raises(NotImplementedError, match="query_closures"):
            bad()


def test_loop_closures_above_signature():
    import inspect
    from sg_pr_amd import sg_net
    sig = inspect.signature(sg_net.SG.loop_closures_above)
    for name in ("seq_slopes", "row_sessions", "col_sessions"):
        assert sig.parameters[name].default is None
    assert sig.parameters["min_terms"].default == 1

    class _Eng:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a, **kw: self.calls.append((name, a, kw))

    class _Self:
        eng = _Eng()

        def engine(self):
            return self.eng

    me = _Self()
    sg_net.SG.loop_closures_above(me, "r", "c", 0.5, window=3)
    sg_net.SG.loop_closures_above(me, "r", "c", 0.5, window=3, seq_len=8)
    sg_net.SG.loop_closures_above(me, "r", "c", 0.5, window=3, seq_len=8, min_terms=4)
    sg_net.SG.loop_closures_above(me, "r", "c", 0.5, seq_len=8, col_sessions=[0, 5], seq_slopes=["1", "2"])
    assert [c[0] for c in me.eng.calls] == ["score_above", "score_seq_above", "score_session_above", "score_session_above"]
    assert me.eng.calls[2][2]["min_terms"] == 4 and me.eng.calls[2][1][4] is None
    assert me.eng.calls[3][1][4].shape == (2, 8) and me.eng.calls[3][2]["col_sessions"] == [0, 5]


# ------------------------------------------------------------------------------------------------- the metric
def test_precision_recall_at_with_col_starts():
    from sg_pr_amd import metrics
    rng = np.random.default_rng(5)
    m = 60
    t = np.arange(m) * 0.35
    xz = np.stack((12.0 * np.cos(t), 12.0 * np.sin(t)), axis=1) + rng.normal(0, 0.3, (m, 2))
    rows = rng.integers(0, m, size=400)
    cols = rng.integers(0, m, size=400)
    d = np.sqrt(((xz[:, None, :] - xz[None, :, :]) ** 2).sum(axis=2))
    rr, cc = np.arange(m)[:, None], np.arange(m)[None, :]
    for starts in ([0], [0, 20, 45], [0, 0, 31]):
        sess = np.searchsorted(np.asarray(starts), np.arange(m), side="right") - 1
        for window in (-1, 0, 7):
            for causal in (False, True):
                ok = np.ones((m, m), dtype=bool)
                if window >= 0:
                    ok &= (np.abs(cc - rr) > window) | (sess[None, :] != sess[:, None])
                if causal:
                    ok &= cc < rr
                positives = int(((d <= 3.0) & ok).sum())
                tp = int((d[rows, cols] <= 3.0).sum())
                fp = int((d[rows, cols] >= 20.0).sum())
                got = metrics.precision_recall_at(rows, cols, xz, p_thresh=3.0, n_thresh=20.0, window=window, causal=causal,
                                                  col_starts=starts)
                assert got == (tp / (tp + fp), tp / positives), (starts, window, causal)
                if len(starts) == 1:                   # one session: today's result, and None is today's call
                    assert got == metrics.precision_recall_at(rows, cols, xz, p_thresh=3.0, n_thresh=20.0, window=window,
                                                              causal=causal)
    # a seam makes the neighbours across it countable
    # 8 frames on a line 10 m apart; frame 4 (the start of session 1) is where frame 3 was, frame 7 where frame 0 was
    line = np.array([[0, 0], [10, 0], [20, 0], [30, 0], [30, 1], [40, 0], [50, 0], [0, 1]], dtype=np.float64)
    assert metrics.precision_recall_at([7, 4], [0, 3], line, window=2) == (1.0, 1.0)       # positives (0, 7), (7, 0)
    assert metrics.precision_recall_at([7, 4], [0, 3], line, window=2, col_starts=[0, 4]) == (1.0, 0.5)   # ... and (3, 4), (4, 3)
    assert metrics.precision_recall_at([7, 4, 2], [0, 3, 6], line, window=2, col_starts=[0, 4], causal=True) == (2 / 3, 1.0)


def test_cli_min_terms_needs_a_threshold():
    from sg_pr_amd import place_db
    with pytest.raises(SystemExit):
        place_db.main(["missing.yml", "--min-terms", "2"])
