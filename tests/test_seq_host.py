"""sgpr_seq_filter / sgpr_score_seq_topk off the GPU: the symbols, the host-side argument checks, the workspace bound,
properties of the NumPy reference (tests/seq_ref.py) and what sequence matching does to a planted revisit.  CPU only."""
import ctypes

import numpy as np
import pytest

import seq_ref


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


FWD, REV, CAUSAL = 2, 4, 1


def test_symbols_present_and_abi_unchanged():
    from sg_pr_amd import engine
    lib = engine.load_library()
    assert lib.sgpr_abi_version() == 11
    for name in ("sgpr_seq_filter", "sgpr_score_seq_topk_workspace_bytes", "sgpr_score_seq_topk"):
        assert name in engine.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    assert (engine.Engine.SEQ_FORWARD, engine.Engine.SEQ_REVERSE, engine.Engine.SEQ_MAX_LEN) == (2, 4, 32)


def test_seq_filter_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host-side checks
    R, M = 100, 300

    def call(h=h, score=p, out=p, dirs=None, r=R, ld=M, ldo=M, ctx=0, L=8, flags=FWD):
        return lib.sgpr_seq_filter(h, score, r, M, ld, ctx, L, flags, out, ldo, dirs, None)

    assert call(h=None) == -1
    assert call(score=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(out=None) == -1
    assert call(ld=M - 1) == -1 and call(ldo=M - 1) == -1
    for L in (0, 33, -1):
        assert call(L=L) == -1 and b"sequence length" in lib.sgpr_last_error()
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
    assert call(flags=0) == -1 and b"direction" in lib.sgpr_last_error()
    assert call(flags=CAUSAL) == -1                  # the causal rule is the selection's, not the filter's
    assert call(flags=FWD | 8) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert call(ctx=R) == 0                          # context rows only: an empty result, nothing launched
    assert call(r=0, score=None, out=None) == 0


def test_score_seq_topk_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)
    R, M = 100, 300
    need = lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, 8, 100, FWD | REV)
    assert need > 0

    def call(h=h, rows=p, cols=p, vals=p, idx=p, dirs=p, flags=FWD | REV, L=8, k=100, ws=p, ws_bytes=need, r=R, row0=0,
             ctx=7):
        return lib.sgpr_score_seq_topk(h, rows, r, cols, M, ctx, None, row0, 10, flags, L, k, vals, idx, dirs, ws,
                                       ws_bytes, None)

    assert call(h=None) == -1
    assert call(rows=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(cols=None) == -1
    assert call(vals=None) == -1
    assert call(idx=None) == -1
    for L in (0, 33, -2):
        assert call(L=L) == -1 and b"sequence length" in lib.sgpr_last_error()
        assert lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, L, 100, FWD) == 0
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
        assert lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, ctx, 8, 100, FWD) == 0
    for flags in (0, CAUSAL):
        assert call(flags=flags) == -1 and b"direction" in lib.sgpr_last_error()
        assert lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, 8, 100, flags) == 0
    assert call(flags=FWD | 8) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, 8, 100, FWD | 8) == 0
    for k in (0, 4097, -3):
        assert call(k=k) == -1 and b"k must" in lib.sgpr_last_error()
        assert lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, 8, k, FWD) == 0
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7
    # every flag combination that is valid has a workspace; one direction needs no dir block
    both = lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, 8, 100, FWD | REV | CAUSAL)
    one = lib.sgpr_score_seq_topk_workspace_bytes(h, R, M, 7, 8, 100, REV | CAUSAL)
    assert 0 < one < both == need
    assert call(ctx=R, ws=None, ws_bytes=0) == 0     # context rows only: an empty result
    assert call(r=0, ctx=0, rows=None, cols=None, vals=None, idx=None, ws=None, ws_bytes=0) == 0
    assert lib.sgpr_score_seq_topk_workspace_bytes(None, R, M, 7, 8, 100, FWD) == 0


def test_seq_workspace_does_not_grow_with_the_matrix():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    fn = lib.sgpr_score_seq_topk_workspace_bytes
    for L in (1, 8, 32):
        big = fn(h, 300000, 300000, L - 1, L, 4096, FWD | REV)
        assert 0 < big < 1e9                          # a 300 k-graph map (a 360 GB matrix)
        for n in (20000, 100000):
            ws, ws2 = fn(h, n, n, 0, L, 1000, FWD | REV | CAUSAL), fn(h, 2 * n, n, 0, L, 1000, FWD | REV | CAUSAL)
            # a 64 MB score block, a Q block and a dir block of its rows (144 MB), plus terms linear in n
            assert 0 < ws < (144 << 20) + 0.02 * 4 * n * n
            assert ws2 - ws < 0.01 * 4 * n * n        # doubling R adds far less than the R x M matrix would
        # one query with its context against a 1 M-frame map: terms linear in M alone (L score rows, one Q row, ...)
        one = fn(h, L, 1 << 20, L - 1, L, 4096, FWD | REV)
        assert 0 < one < (L + 2) * 4 * (1 << 20) + 256 * (1 << 20)


# ------------------------------------------------------------------------------------------------- the reference itself
def _random_scores(r, m, seed):
    rng = np.random.default_rng(seed)
    s = rng.random((r, m), dtype=np.float32)
    s[rng.random((r, m)) < 0.02] = np.nan
    s[rng.random((r, m)) < 0.01] = -0.0
    s[rng.random((r, m)) < 0.01] = np.inf
    return s


def test_reference_length_one_forward_is_the_identity():
    s = _random_scores(23, 41, 0)
    for ctx in (0, 5, 23):
        q, d = seq_ref.seq_filter(s, 1, ctx=ctx, forward=True, reverse=False)
        assert q.shape == (23 - ctx, 41) and d.shape == q.shape
        assert np.array_equal(q.view(np.uint32), s[ctx:].view(np.uint32))     # bit for bit, NaN and -0.0 included
        assert not d.any()
    q, d = seq_ref.seq_filter(s, 1, forward=False, reverse=True)
    assert np.array_equal(q.view(np.uint32), s.view(np.uint32)) and d.all()


def test_reference_term_counts_at_the_four_edges():
    r, m, L = 9, 13, 4
    ones = np.ones((r, m), dtype=np.float32)
    # a matrix of ones averages to exactly 1 whatever the count; a matrix of row + column indices shows the count
    for fwd, rev in ((True, False), (False, True)):
        q, _ = seq_ref.seq_filter(ones, L, forward=fwd, reverse=rev)
        assert np.array_equal(q, ones)
    nf, nr = seq_ref.term_counts(r, m, L, +1), seq_ref.term_counts(r, m, L, -1)
    assert nf[0].tolist() == [1] * m and nr[0].tolist() == [1] * m            # top edge: the d = 0 term alone
    assert nf[:, 0].tolist() == [1] * r and nr[:, m - 1].tolist() == [1] * r  # forward at the left, reverse at the right
    assert nf[r - 1].tolist() == [1, 2, 3] + [4] * (m - 3)                    # bottom edge: the column limits alone
    assert nr[r - 1].tolist() == [4] * (m - 3) + [3, 2, 1]
    assert nf[:, m - 1].tolist() == [1, 2, 3] + [4] * (r - 3)                 # the far column: the row limit alone
    assert nr[:, 0].tolist() == [1, 2, 3] + [4] * (r - 3)
    # ... and the sums are those of exactly these terms: S = 2^r (sums of distinct powers of two name their terms)
    s = np.repeat((2.0 ** np.arange(r))[:, None], m, axis=1).astype(np.float32)
    for sigma, n in ((+1, nf), (-1, nr)):
        q, _ = seq_ref.seq_filter(s, L, forward=sigma > 0, reverse=sigma < 0)
        for rr in range(r):
            for cc in range(m):
                want = np.float32(sum(2.0 ** (rr - d) for d in range(n[rr, cc]))) * seq_ref.RCP[n[rr, cc]]
                assert q[rr, cc] == want, (sigma, rr, cc)
    # L larger than both sides
    q, _ = seq_ref.seq_filter(ones[:3, :2], 32, forward=True, reverse=True)
    assert np.array_equal(q, ones[:3, :2])
    assert seq_ref.RCP[3] == np.float32(1.0 / 3.0) and seq_ref.RCP[32] == np.float32(0.03125)


def test_reference_forward_wins_ties():
    s = np.full((6, 6), 0.5, dtype=np.float32)
    q, d = seq_ref.seq_filter(s, 3, forward=True, reverse=True)
    assert np.array_equal(q, s) and not d.any()                # equal everywhere: forward
    s[2, 4] = 0.75                                             # lifts the reverse sum of (3, 3) and the forward sum of (3, 5)
    q, d = seq_ref.seq_filter(s, 3, forward=True, reverse=True)
    assert d[3, 3] == 1 and d[3, 5] == 0
    assert d[4, 2] == 1                                        # (4, 2) reaches it at d = 2
    assert d[2, 4] == 1 and d.sum() == 3                       # at (2, 4) itself the reverse mean has two terms, not three
    s[:] = 0.5
    s[1, 1] = np.nan                                           # forward of (2, 2) is NaN, its reverse is not
    q, d = seq_ref.seq_filter(s, 2, forward=True, reverse=True)
    assert d[2, 2] == 1 and q[2, 2] == 0.5
    assert np.isnan(q[1, 1]) and d[1, 1] == 1                  # both NaN: the rule says reverse (forward is NaN)
    assert q[2, 0] == 0.5 and d[2, 0] == 0                     # reverse of (2, 0) is NaN, forward (one term) is not


# ------------------------------------------------------------------------------------------------- the planted case
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_revisits(seed):
    s, col = seq_ref.planted(seed)
    one_f, one_r = seq_ref.planted_rates(s, col)
    print("seed", seed, "L = 1:", one_f, one_r)
    qf, _ = seq_ref.seq_filter(s, 8, forward=True, reverse=False)
    qr, _ = seq_ref.seq_filter(s, 8, forward=False, reverse=True)
    qb, db = seq_ref.seq_filter(s, 8, forward=True, reverse=True)
    ff, fr = seq_ref.planted_rates(qf, col)
    rf, rr = seq_ref.planted_rates(qr, col)
    bf, br = seq_ref.planted_rates(qb, col)
    print("seed", seed, "L = 8 forward filter:", ff, fr, "reverse filter:", rf, rr, "both:", bf, br)
    assert one_f <= 0.55 and one_r <= 0.55                     # single scans: the lift is lost in the noise half the time
    assert ff >= 0.90 and rr >= 0.90                           # the matching direction finds the run
    assert fr <= 0.05 and rf <= 0.05                           # the opposite one sees one lifted term in eight
    assert bf >= 0.85 and br >= 0.85
    rows_f, rows_r = np.arange(208, 300), np.arange(308, 400)
    assert not db[rows_f, col[rows_f]].any() and db[rows_r, col[rows_r]].all()
