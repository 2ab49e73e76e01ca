"""sgpr_seq_path_filter / sgpr_score_path_topk off the GPU: the symbols, the host-side argument checks, the workspace
identities, properties of the NumPy reference (tests/seq_path_ref.py) and of engine.seq_paths, and what a path set does
to a planted revisit of another slope.  CPU only."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import seq_path_ref
import seq_ref

FWD, REV, CAUSAL = 2, 4, 1


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


def _table(paths):
    t = np.ascontiguousarray(paths, dtype=np.int32)
    return t, ctypes.c_void_p(t.ctypes.data)


def test_symbols_present_and_abi_unchanged():
    from sg_pr_amd import engine
    lib = engine.load_library()
    assert lib.sgpr_abi_version() == 11
    for name in ("sgpr_seq_path_filter", "sgpr_score_path_topk_workspace_bytes", "sgpr_score_path_topk"):
        assert name in engine.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    assert (engine.Engine.SEQ_MAX_PATHS, engine.Engine.SEQ_PATH_MAX_OFFSET) == (16, 64)
    assert (seq_path_ref.MAX_PATHS, seq_path_ref.MAX_OFFSET) == (16, 64)


def _bad_tables(L):
    """(table, word of the message) for every fault of a path table"""
    unit = np.arange(L, dtype=np.int32)
    start = unit.copy()
    start[0] = 1
    down = unit.copy()
    down[L // 2] = down[L // 2 - 1] - 1
    far = np.zeros(L, dtype=np.int32)
    far[L - 1] = 65
    neg = unit.copy()
    neg[1:] = -1
    return [(np.stack([unit, start]), b"start"), (np.stack([unit, down]), b"decreasing"), (np.stack([far]), b"above 64"),
            (np.stack([unit, neg]), b"decreasing")]


def test_seq_path_filter_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300
    good, good_p = _table(seq_path_ref.seq_paths(8, seq_path_ref.SLOPES))

    def call(h=h, score=p, out=p, code=None, r=R, ld=M, ldo=M, ctx=0, L=8, flags=FWD, table=good_p, n=good.shape[0]):
        return lib.sgpr_seq_path_filter(h, score, r, M, ld, ctx, L, flags, table, n, out, ldo, code, None)

    assert call(h=None) == -1
    assert call(score=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(out=None) == -1
    assert call(ld=M - 1) == -1 and call(ldo=M - 1) == -1
    for L in (0, 33, -1):
        assert call(L=L) == -1 and b"sequence length" in lib.sgpr_last_error()
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
    assert call(flags=0) == -1 and b"direction" in lib.sgpr_last_error()
    assert call(flags=CAUSAL) == -1
    assert call(flags=FWD | 8) == -1 and b"flag" in lib.sgpr_last_error()
    for n in (0, 17, -1):
        assert call(n=n) == -1 and b"n_paths" in lib.sgpr_last_error()
    assert call(table=None) == -1 and b"NULL path table" in lib.sgpr_last_error()
    for bad, word in _bad_tables(8):
        t, tp = _table(bad)
        assert call(table=tp, n=t.shape[0]) == -1 and word in lib.sgpr_last_error(), (bad, lib.sgpr_last_error())
    edge = np.zeros((1, 8), dtype=np.int32)
    edge[0, 7] = 64                                  # the largest offset allowed: passes the table check (ctx == R: no launch)
    t, tp = _table(edge)
    assert call(table=tp, n=1, ctx=R) == 0
    assert call(ctx=R) == 0                          # context rows only: an empty result, nothing launched
    assert call(r=0, score=None, out=None) == 0


def test_score_path_topk_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)
    R, M = 100, 300
    good, good_p = _table(seq_path_ref.seq_paths(8, seq_path_ref.SLOPES))
    P = good.shape[0]
    wsb = lib.sgpr_score_path_topk_workspace_bytes
    need = wsb(h, R, M, 7, 8, P, 100, 10, FWD | REV)
    assert need > 0

    def call(h=h, rows=p, cols=p, vals=p, idx=p, codes=p, flags=FWD | REV, L=8, k=100, ws=p, ws_bytes=need, r=R, row0=0,
             ctx=7, table=good_p, n=P, radius=10):
        return lib.sgpr_score_path_topk(h, rows, r, cols, M, ctx, None, row0, 10, flags, L, table, n, radius, k, vals, idx,
                                        codes, ws, ws_bytes, None)

    assert call(h=None) == -1
    assert call(rows=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(cols=None) == -1
    assert call(vals=None) == -1
    assert call(idx=None) == -1
    for L in (0, 33, -2):
        assert call(L=L) == -1 and b"sequence length" in lib.sgpr_last_error()
        assert wsb(h, R, M, 7, L, P, 100, 10, FWD) == 0
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
        assert wsb(h, R, M, ctx, 8, P, 100, 10, FWD) == 0
    for flags in (0, CAUSAL):
        assert call(flags=flags) == -1 and b"direction" in lib.sgpr_last_error()
        assert wsb(h, R, M, 7, 8, P, 100, 10, flags) == 0
    assert call(flags=FWD | 8) == -1 and b"flag" in lib.sgpr_last_error()
    assert wsb(h, R, M, 7, 8, P, 100, 10, FWD | 8) == 0
    for k in (0, 4097, -3):
        assert call(k=k) == -1 and b"k must" in lib.sgpr_last_error()
        assert wsb(h, R, M, 7, 8, P, k, 10, FWD) == 0
    for radius in (-1, 1025):
        assert call(radius=radius) == -1 and b"radius" in lib.sgpr_last_error()
        assert wsb(h, R, M, 7, 8, P, 100, radius, FWD) == 0
    for n in (0, 17, -1):
        assert call(n=n) == -1 and b"n_paths" in lib.sgpr_last_error()
        assert wsb(h, R, M, 7, 8, n, 100, 10, FWD) == 0
    assert call(table=None) == -1 and b"NULL path table" in lib.sgpr_last_error()
    for bad, word in _bad_tables(8):
        t, tp = _table(bad)
        assert call(table=tp, n=t.shape[0]) == -1 and word in lib.sgpr_last_error(), (bad, lib.sgpr_last_error())
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7
    assert call(ctx=R, ws=None, ws_bytes=0) == 0     # context rows only: an empty result
    assert call(r=0, ctx=0, rows=None, cols=None, vals=None, idx=None, ws=None, ws_bytes=0) == 0
    assert wsb(None, R, M, 7, 8, P, 100, 10, FWD) == 0


def test_workspace_identities():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    wsb = lib.sgpr_score_path_topk_workspace_bytes
    a256 = lambda v: (v + 255) & ~255
    for R, M in ((100, 300), (300, 517), (20000, 20000), (150, 262144)):
        for L in (1, 8, 32):
            rb = max(1, min(R, (64 << 20) // (4 * M) - (L - 1)))
            for k in (1, 100):
                for flags in (FWD, REV | CAUSAL, FWD | REV, FWD | REV | CAUSAL):
                    ctx = min(L - 1, R)
                    # 1. the unit path, radius 0: sgpr_score_seq_topk's workspace
                    seq = lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, ctx, L, k, flags)
                    assert wsb(h, R, M, ctx, L, 1, k, 0, flags) == seq > 0
                    # 2. the unit path, radius > 0: sgpr_score_peak_topk's
                    for radius in (1, 10, 1024):
                        peak = lib.sgpr_score_peak_topk_workspace_bytes(h, R, M, ctx, L, k, radius, flags)
                        assert wsb(h, R, M, ctx, L, 1, k, radius, flags) == peak > 0
                    # 3. several paths: one code block more with one direction, nothing more with both (the dir block)
                    grow = 0 if (flags & FWD) and (flags & REV) else a256(rb * M)
                    for n in (2, 9, 16):
                        assert wsb(h, R, M, ctx, L, n, k, 0, flags) == seq + grow
                        assert wsb(h, R, M, ctx, L, n, k, 10, flags) == \
                            lib.sgpr_score_peak_topk_workspace_bytes(h, R, M, ctx, L, k, 10, flags) + grow
    # never R x M: a 300 k-graph map (a 360 GB matrix)
    assert 0 < wsb(h, 300000, 300000, 31, 32, 16, 4096, 1024, FWD) < 1e9


# ------------------------------------------------------------------------------------------------- the reference itself
def _random_scores(r, m, seed):
    rng = np.random.default_rng(seed)
    s = np.round(rng.random((r, m), dtype=np.float32) * 64.0) / np.float32(64.0)      # quantised: ties occur
    s[rng.random((r, m)) < 0.02] = np.nan
    s[rng.random((r, m)) < 0.01] = -0.0
    s[rng.random((r, m)) < 0.01] = np.inf
    s[rng.random((r, m)) < 0.01] = -np.inf
    return s.astype(np.float32)


@pytest.mark.parametrize("L", [1, 2, 8, 32])
def test_reference_unit_path_is_the_diagonal_filter(L):
    for r, m in ((1, 1), (5, 7), (40, 70), (70, 33)):
        s = _random_scores(r, m, 11 * r + m)
        for fwd, rev in ((True, False), (False, True), (True, True)):
            for ctx in sorted({0, min(L - 1, r), r}):
                wq, wd = seq_ref.seq_filter(s, L, ctx, fwd, rev)
                q, c = seq_path_ref.path_filter(s, seq_path_ref.unit_path(L), ctx, fwd, rev)
                assert q.shape == wq.shape and c.dtype == np.uint8
                assert np.array_equal(q.view(np.uint32), wq.view(np.uint32)), (L, r, m, fwd, rev, ctx)
                assert np.array_equal(c, wd), (L, r, m, fwd, rev, ctx)
                # duplicate paths change nothing: the first of equal candidates stays
                q2, c2 = seq_path_ref.path_filter(s, np.repeat(seq_path_ref.unit_path(L), 16, axis=0), ctx, fwd, rev)
                assert np.array_equal(q2.view(np.uint32), wq.view(np.uint32))
                keep = ~np.isnan(wq)                 # (a NaN best is replaced by every later candidate: the last one)
                assert np.array_equal(c2[keep], wd[keep])


def test_reference_terms_and_fold():
    # S = 2^r names the rows of a sum, S = 2^c the columns: the path (0, 0, 2, 5) forward from (5, 9)
    r, m = 8, 12
    off = np.array([[0, 0, 2, 5]], dtype=np.int32)
    rows = np.repeat((2.0 ** np.arange(r))[:, None], m, axis=1).astype(np.float32)
    cols = np.repeat((2.0 ** np.arange(m))[None, :], r, axis=0).astype(np.float32)
    q, c = seq_path_ref.path_filter(rows, off, 0, True, False)
    assert q[5, 9] == np.float32(2.0 ** 5 + 2.0 ** 4 + 2.0 ** 3 + 2.0 ** 2) * seq_path_ref.RCP[4] and c[5, 9] == 0
    q, _ = seq_path_ref.path_filter(cols, off, 0, True, False)
    assert q[5, 9] == np.float32(2.0 ** 9 + 2.0 ** 9 + 2.0 ** 7 + 2.0 ** 4) * seq_path_ref.RCP[4]
    assert q[5, 4] == np.float32(2.0 ** 4 + 2.0 ** 4 + 2.0 ** 2) * seq_path_ref.RCP[3]       # 4 - 5 < 0: a prefix of 3
    assert q[5, 1] == np.float32(2.0 ** 1 + 2.0 ** 1) * seq_path_ref.RCP[2]
    assert q[1, 9] == np.float32(2.0 ** 9 + 2.0 ** 9) * seq_path_ref.RCP[2]                   # the row limit
    q, c = seq_path_ref.path_filter(cols, off, 0, False, True)
    assert q[5, 2] == np.float32(2.0 ** 2 + 2.0 ** 2 + 2.0 ** 4 + 2.0 ** 7) * seq_path_ref.RCP[4] and c[5, 2] == 1
    assert q[5, 8] == np.float32(2.0 ** 8 + 2.0 ** 8 + 2.0 ** 10) * seq_path_ref.RCP[3]       # 8 + 5 >= 12
    # the fold: the first of equal candidates wins, a NaN best is replaced, code = direction bit | path << 1
    s = np.full((6, 9), 0.5, dtype=np.float32)
    two = np.array([[0, 1, 2], [0, 2, 4]], dtype=np.int32)
    q, c = seq_path_ref.path_filter(s, two, 0, True, True)
    assert np.array_equal(q, s) and not c.any()
    s[3, 4] = 0.75                                   # lifts path 1 forward at (4, 6), path 0 reverse at (4, 3), ...
    q, c = seq_path_ref.path_filter(s, two, 0, True, True)
    assert c[4, 6] == 2 and c[4, 5] == 0 and c[4, 3] == 1 and c[4, 2] == 3 and c[5, 6] == 0 and c[5, 8] == 2
    s[:] = 0.5
    s[3, 4] = np.nan
    q, c = seq_path_ref.path_filter(s, two, 0, True, True)
    assert c[4, 5] == 2 and q[4, 5] == 0.5           # path 0 forward is NaN: the next candidate replaces it
    assert np.isnan(q[3, 4]) and c[3, 4] == 3        # every candidate NaN: the last one


def test_seq_paths():
    from sg_pr_amd import engine
    for fn in (engine.seq_paths, seq_path_ref.seq_paths):
        t = fn(8, ["1"])
        assert t.dtype == np.int32 and t.tolist() == [list(range(8))]
        # phases: slope 1/2 has two, slope 2/3 three; (p, q), Fraction and string forms agree
        assert fn(5, [(1, 2)]).tolist() == [[0, 0, 1, 1, 2], [0, 1, 1, 2, 2]]
        assert fn(5, [Fraction(2, 3)]).tolist() == [[0, 0, 1, 2, 2], [0, 1, 1, 2, 3], [0, 1, 2, 2, 3]]
        assert fn(5, ["3/2"]).tolist() == [[0, 1, 3, 4, 6], [0, 2, 3, 5, 6]]
        assert np.array_equal(fn(7, ["2/4", (3, 2)]), fn(7, [Fraction(1, 2), "3/2"]))
        # de-duplication in order: at L = 2 slope 1/2's second phase is slope 1, slope 2/3's phases are both of them
        assert fn(2, ["1/2", "1", "2/3", "2"]).tolist() == [[0, 0], [0, 1], [0, 2]]
        assert fn(1, seq_path_ref.SLOPES).tolist() == [[0]]
        for L, far in ((8, 14), (16, 30)):
            t = fn(L, seq_path_ref.SLOPES)
            assert t.shape == (9, L) and t.max() == far
            assert (t[:, 0] == 0).all() and (np.diff(t, axis=1) >= 0).all()
            assert len({tuple(p) for p in t.tolist()}) == 9
        # the limits
        assert fn(17, ["4"]).max() == 64
        with pytest.raises(ValueError):
            fn(17, ["65/16"])                        # 16 phases, each 65 columns in 16 steps
        with pytest.raises(ValueError):
            fn(8, ["10"])                            # 70 columns in 7 steps
        assert fn(32, ["1/16"]).shape == (16, 32)
        with pytest.raises(ValueError):
            fn(32, ["1/17"])                         # 17 phases
        with pytest.raises(ValueError):
            fn(32, ["1/16", "1"])
    assert np.array_equal(engine.seq_paths(16, seq_path_ref.SLOPES), seq_path_ref.seq_paths(16, seq_path_ref.SLOPES))


# ------------------------------------------------------------------------------------------------- the planted case
PLANTED_SLOPES = [(2, 1), (1, 2), (3, 2), (2, 3)]


def planted_figures(s, col, unit_q, path_q, path_code, L=8, window=50):
    """(unit forward, unit reverse, path forward, path reverse, share of planted entries with the right direction bit)
    over the rows at least L into each revisit"""
    uf, ur = seq_ref.planted_rates(unit_q, col, window=window, skip=L)
    pf, pr = seq_ref.planted_rates(path_q, col, window=window, skip=L)
    fwd, rev = np.arange(200 + L, 300), np.arange(300 + L, 400)
    right = np.concatenate([(path_code[fwd, col[fwd]] & 1) == 0, (path_code[rev, col[rev]] & 1) == 1])
    return uf, ur, pf, pr, float(right.mean())


@pytest.mark.parametrize("slope", PLANTED_SLOPES, ids=["%d/%d" % s for s in PLANTED_SLOPES])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_revisits_of_another_slope(seed, slope):
    L = 8
    s, col = seq_path_ref.planted(seed, slope)
    paths = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    unit_q = seq_ref.seq_filter(s, L, 0, True, True)[0]
    q, code = seq_path_ref.path_filter(s, paths, 0, True, True)
    uf, ur, pf, pr, right = planted_figures(s, col, unit_q, q, code, L)
    print("seed", seed, "slope", slope, "unit diagonal:", uf, ur, "path set:", pf, pr, "direction bit right:", right)
    assert uf <= 0.15 and ur <= 0.15                 # the unit diagonal: one true score in eight
    assert pf >= 0.75 and pr >= 0.75                 # the path set holds the slope
    # the reference alone, to the two decimals its figures are quoted with (0.00 - 0.08 and 0.82 - 0.99; the lowest,
    # seed 0 slope 2 reverse, is 75 of 92 rows = 0.815)
    assert max(round(uf, 2), round(ur, 2)) <= 0.08 and min(round(pf, 2), round(pr, 2)) >= 0.82
    assert right >= 0.95
