"""sgpr_peak_filter / sgpr_score_peak_topk off the GPU: the symbols, the host-side argument checks, the workspace bound,
properties of the NumPy reference (tests/peak_ref.py) and what the peak filter does to a planted row.  CPU only."""
import ctypes

import numpy as np
import pytest

import peak_ref


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


FWD, REV, CAUSAL = 2, 4, 1


def test_symbols_present_and_abi_unchanged():
    from sg_pr_amd import _build, engine
    lib = engine.load_library()
    assert lib.sgpr_abi_version() == 11
    with open(_build.HEADERS[0]) as f:
        header = f.read()
    for name in ("sgpr_peak_filter", "sgpr_score_peak_topk_workspace_bytes", "sgpr_score_peak_topk"):
        assert name + "(" in header
        assert name in engine.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    assert "#define SGPR_PEAK_MAX_RADIUS 1024" in header and "#define SGPR_PEAK_STRIP 1024" in header
    assert (engine.Engine.PEAK_MAX_RADIUS, engine.Engine.PEAK_STRIP) == (1024, 1024)
    assert peak_ref.MAX_RADIUS == engine.Engine.PEAK_MAX_RADIUS
    for name in ("peak_filter", "score_peak_topk", "score_peak_topk_workspace_bytes"):
        assert callable(getattr(engine.Engine, name))


def test_peak_filter_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300

    def call(h=h, score=p, out=p, r=R, ld=M, ldo=M, row0=0, window=10, flags=0, radius=5):
        return lib.sgpr_peak_filter(h, score, r, M, ld, None, row0, window, flags, radius, out, ldo, None)

    assert call(h=None) == -1
    assert call(score=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(out=None) == -1
    assert call(ld=M - 1) == -1 and call(ldo=M - 1) == -1
    assert call(r=-1) == -1
    assert call(window=-2) == -1 and b"window" in lib.sgpr_last_error()
    for radius in (-1, 1025, 1 << 30):
        assert call(radius=radius) == -1 and b"radius" in lib.sgpr_last_error()
    for flags in (FWD, REV, 8, -1):                  # the directions are the sequence filter's, not the peak filter's
        assert call(flags=flags) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(r=0, score=None, out=None) == 0      # an empty result, nothing launched


def test_score_peak_topk_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)
    R, M = 100, 300
    ws_fn = lib.sgpr_score_peak_topk_workspace_bytes
    need = ws_fn(h, R, M, 7, 8, 100, 5, FWD | REV)
    assert need > 0

    def call(h=h, rows=p, cols=p, vals=p, idx=p, dirs=p, flags=FWD | REV, L=8, k=100, ws=p, ws_bytes=need, r=R, row0=0,
             ctx=7, radius=5):
        return lib.sgpr_score_peak_topk(h, rows, r, cols, M, ctx, None, row0, 10, flags, L, radius, k, vals, idx, dirs,
                                        ws, ws_bytes, None)

    assert call(h=None) == -1
    assert call(rows=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(cols=None) == -1
    assert call(vals=None) == -1
    assert call(idx=None) == -1
    for L in (0, 33, -2):
        assert call(L=L) == -1 and b"sequence length" in lib.sgpr_last_error()
        assert ws_fn(h, R, M, 7, L, 100, 5, FWD) == 0
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
        assert ws_fn(h, R, M, ctx, 8, 100, 5, FWD) == 0
    for flags in (0, CAUSAL):
        assert call(flags=flags) == -1 and b"direction" in lib.sgpr_last_error()
        assert ws_fn(h, R, M, 7, 8, 100, 5, flags) == 0
    assert call(flags=FWD | 8) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert ws_fn(h, R, M, 7, 8, 100, 5, FWD | 8) == 0
    for k in (0, 4097, -3):
        assert call(k=k) == -1 and b"k must" in lib.sgpr_last_error()
        assert ws_fn(h, R, M, 7, 8, k, 5, FWD) == 0
    for radius in (-1, 1025, 1 << 30):               # the new rule
        assert call(radius=radius) == -1 and b"radius" in lib.sgpr_last_error()
        assert ws_fn(h, R, M, 7, 8, 100, radius, FWD) == 0
    assert call(radius=0, ws_bytes=0) == -7 and call(radius=1024, ws_bytes=0) == -7   # both ends are valid radii
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7
    # one direction needs no dir block, L = 1 neither a Q block nor a dir block; the radius does not enter
    both = ws_fn(h, R, M, 7, 8, 100, 5, FWD | REV | CAUSAL)
    one = ws_fn(h, R, M, 7, 8, 100, 5, REV | CAUSAL)
    single = ws_fn(h, R, M, 0, 1, 100, 5, FWD | REV)
    assert 0 < single < one < both == need
    assert ws_fn(h, R, M, 7, 8, 100, 0, FWD | REV) == ws_fn(h, R, M, 7, 8, 100, 1024, FWD | REV) == need
    # ... and it is sgpr_score_seq_topk's plus one P block of the same rows
    p_block = (R * M * 4 + 255) & ~255
    assert need == lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, 8, 100, FWD | REV) + p_block
    assert call(ctx=R, ws=None, ws_bytes=0) == 0     # context rows only: an empty result
    assert call(r=0, ctx=0, rows=None, cols=None, vals=None, idx=None, ws=None, ws_bytes=0) == 0
    assert ws_fn(None, R, M, 7, 8, 100, 5, FWD) == 0


def test_peak_workspace_does_not_grow_with_the_matrix():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    fn = lib.sgpr_score_peak_topk_workspace_bytes
    for L in (1, 8, 32):
        big = fn(h, 300000, 300000, L - 1, L, 4096, 50, FWD | REV)
        assert 0 < big < 1e9                          # a 300 k-graph map (a 360 GB matrix)
        for n in (20000, 100000):
            ws, ws2 = fn(h, n, n, 0, L, 1000, 50, FWD | REV | CAUSAL), fn(h, 2 * n, n, 0, L, 1000, 50, FWD | REV | CAUSAL)
            # a 64 MB score block, a P block, a Q block and a dir block of its rows (208 MB), plus terms linear in n
            assert 0 < ws < (208 << 20) + 0.02 * 4 * n * n
            assert ws2 - ws < 0.01 * 4 * n * n        # doubling R adds far less than the R x M matrix would


# ------------------------------------------------------------------------------------------------- the reference itself
def _quantised(seed, r=8, m=300, levels=16):
    """ties everywhere; a few NaN, -inf, +inf and -0.0"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, levels, size=(r, m)) / np.float32(levels)).astype(np.float32)
    for val, frac in ((np.nan, 0.02), (-np.inf, 0.02), (np.inf, 0.005), (-0.0, 0.02)):
        x[rng.random((r, m)) < frac] = val
    return x


MODES = [dict(), dict(window=0), dict(window=20), dict(window=20, causal=True), dict(window=-1, causal=True, row0=150),
         dict(window=5, row_self=np.array([0, 299, 150, 7, 290, 100, 33, 200]))]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_properties(seed):
    x = _quantised(seed)
    for mode in MODES:
        ok = peak_ref.qualifies(x, **mode)
        for rho in (0, 1, 3, 10, 299, 1024):
            pk = peak_ref.peaks(x, rho, **mode)
            if rho in (1, 10):
                assert np.array_equal(pk, peak_ref.peaks_slow(x, rho, **mode)), (mode, rho)   # the two forms of the loop
            assert not (pk & ~ok).any()                             # only qualifying columns
            for r in range(x.shape[0]):
                cols = np.flatnonzero(pk[r])
                assert (np.diff(cols) > rho).all(), (mode, rho, r)  # peaks are more than rho apart
                if ok[r].any():                                     # the row maximum (its first column) is a peak
                    best = peak_ref.lists(x[r:r + 1], 1, **_row(mode, r))[1][0, 0]
                    assert pk[r, best], (mode, rho, r)
                else:
                    assert not pk[r].any()
            if rho == 0:                                            # rho = 0: the plain lists
                assert np.array_equal(pk, ok)
                for k in (1, 4, 400):
                    got, want = peak_ref.peak_lists(x, 0, k, **mode), peak_ref.lists(x, k, **mode)
                    assert np.array_equal(got[1], want[1])
                    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
            # a column that does not qualify suppresses nothing: replacing it by NaN changes no peak
            y = np.where(ok, x, np.float32(np.nan))
            assert np.array_equal(peak_ref.peaks(y, rho), pk)


def _row(mode, r):
    """the mode of row r taken on its own"""
    out = {k: v for k, v in mode.items() if k not in ("row_self", "row0")}
    out["row0"] = int(mode["row_self"][r]) if "row_self" in mode else mode.get("row0", 0) + r
    return out


def test_reference_lists_by_hand():
    inf, nan = np.inf, np.nan
    #                 0    1    2     3    4    5    6     7    8
    x = np.array([[0.5, 0.5, 0.25, nan, 0.5, 0.0, -0.0, -inf, inf]], dtype=np.float32)
    v, i = peak_ref.lists(x, 9)
    assert i.tolist() == [[8, 0, 1, 4, 2, 5, 6, -1, -1]]                   # -0.0 ties +0.0: the lower column first
    assert np.signbit(v[0, 6]) and not np.signbit(v[0, 5])                 # the stored bits
    assert v[0, 7] == -inf and v[0, 0] == inf
    # rho = 1: 0 beats 1 (equal, lower column); 4 stands beside a NaN and the zero at 5; 8 beats nothing that qualifies
    assert np.flatnonzero(peak_ref.peaks(x, 1)[0]).tolist() == [0, 4, 8]
    assert np.flatnonzero(peak_ref.peaks(x, 2)[0]).tolist() == [0, 4, 8]   # 2 loses to 0 and 4, 6 to 4 and 8
    assert np.flatnonzero(peak_ref.peaks(x, 3)[0]).tolist() == [0, 8]      # 4 loses to 1 (equal, lower column) - not a
    # peak itself: "first in its neighbourhood", not "not beaten by a peak"
    assert np.flatnonzero(peak_ref.peaks(x, 4)[0]).tolist() == [0, 8]
    # a plateau longer than rho: its first column only
    flat = np.full((1, 30), 0.5, dtype=np.float32)
    assert np.flatnonzero(peak_ref.peaks(flat, 4)[0]).tolist() == [0]
    # ... unless what stands before it does not qualify: window 2 around frame 10 cuts columns 8..12
    assert np.flatnonzero(peak_ref.peaks(flat, 4, window=2, row0=10)[0]).tolist() == [0, 13]
    # causal: the columns from self_r on do not exist for the row
    assert np.flatnonzero(peak_ref.peaks(flat, 4, causal=True, row0=0)[0]).tolist() == []
    v, i = peak_ref.peak_lists(flat, 4, 3, window=2, row0=10)
    assert i.tolist() == [[0, 13, -1]] and v.tolist() == [[0.5, 0.5, -inf]]
    assert peak_ref.places_per_list(np.array([[5, 6, 7, 30, -1], [1, 100, 200, 2, 3], [-1] * 5]), 10) == 2.5


def test_reference_causal_prefix_equals_offline():
    """A causal query that knows only the columns c < self_r gets the lists of the offline call."""
    x = _quantised(5, r=40, m=40)
    for rho, window in ((3, -1), (3, 5), (10, 2)):
        off = peak_ref.peak_lists(x, rho, 3, window=window, causal=True)
        for t in range(40):
            on = peak_ref.peak_lists(x[t:t + 1, :t], rho, 3, window=window, causal=True, row0=t)
            assert np.array_equal(on[1], off[1][t:t + 1]) and np.array_equal(on[0].view(np.uint32),
                                                                              off[0][t:t + 1].view(np.uint32))


# ------------------------------------------------------------------------------------------------- the planted case
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_bumps(seed):
    x = peak_ref.planted(seed)
    assert x.shape == (1, 400)
    for centre in (100, 200, 300):                  # noise cannot move a centre
        assert x[0, centre] - max(x[0, centre - 1], x[0, centre + 1]) > 0.0038
    plain = peak_ref.lists(x, 4)[1][0]
    assert (np.abs(plain - 100) <= 2).all()          # the plain top-4 is one place seen four times
    assert peak_ref.places_per_list(plain[None, :], 10) == 1.0
    v, i = peak_ref.peak_lists(x, 10, 3)
    assert i[0].tolist() == [100, 200, 300]          # the distinct top-3: the three places
    assert np.array_equal(v[0], x[0, [100, 200, 300]])
    assert peak_ref.places_per_list(i, 10) == 3.0
