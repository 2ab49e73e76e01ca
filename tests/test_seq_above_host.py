"""sgpr_seq_rows_above / sgpr_score_seq_above / sgpr_score_seq_positives / sgpr_score_seq_threshold_counts off the GPU:
the symbols, the host-side argument checks, the workspace bounds, and what thresholding the sequence-matched score does
to a planted revisit (tests/seq_above_ref.py).  CPU only."""
import ctypes
import struct

import numpy as np
import pytest

import seq_above_ref
import seq_ref

FWD, REV, CAUSAL = 2, 4, 1
NAMES = ("sgpr_seq_rows_above", "sgpr_score_seq_above", "sgpr_score_seq_positives", "sgpr_score_seq_threshold_counts")
M_A = 4541
RB_A = (64 << 20) // (4 * M_A)              # rows of a 64 MB score block at M_A columns (test_gpu_row_blocks.RB_A)


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    from sg_pr_amd import engine
    return engine.load_library()


def test_symbols_present_and_abi_unchanged(lib):
    from sg_pr_amd import engine
    assert lib.sgpr_abi_version() == 11
    for name in NAMES:
        for sym in (name, name + "_workspace_bytes"):
            assert sym in engine.ABI_SYMBOLS
            assert getattr(lib, sym) is not None
    for method in ("seq_rows_above", "score_seq_above", "score_seq_positives", "score_seq_threshold_counts"):
        assert callable(getattr(engine.Engine, method))
        assert callable(getattr(engine.Engine, method + "_workspace_bytes"))


R, M = 100, 300
P = ctypes.c_void_p(4096)                            # never dereferenced: every call below fails its host-side checks
NAN, INF = float("nan"), float("inf")


def _above_checks(lib, call, query):
    assert call(h=None) == -1
    assert call(count=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(src=None) == -1 and b"NULL" in lib.sgpr_last_error()
    for L in (0, 33, -1):
        assert call(L=L) == -1 and b"sequence length" in lib.sgpr_last_error()
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
    for flags in (0, CAUSAL):
        assert call(flags=flags) == -1 and b"direction" in lib.sgpr_last_error()
    assert call(flags=FWD | 8) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=-1) == -1
    assert call(thr=NAN) == -1 and b"NaN" in lib.sgpr_last_error()
    assert call(cap=-1) == -1 and b"capacity" in lib.sgpr_last_error()
    for missing in ("rows", "cols", "vals"):
        assert call(**{missing: None}) == -1            # capacity without arrays
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    need = query()
    assert need > 0
    assert call(ws_bytes=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert call(ws=None) == -7


def test_seq_rows_above_argument_checks_touch_no_device(lib):
    keep, h = _zeroed_handle()
    fn = lib.sgpr_seq_rows_above_workspace_bytes
    need = fn(h, R, M, 7)

    def call(h=h, src=P, r=R, m=M, ld=M, ctx=7, flags=FWD | REV, L=8, thr=0.5, rows=P, cols=P, vals=P, dirs=P, cap=10,
             row_ptr=P, count=P, ws=P, ws_bytes=need, row0=0):
        return lib.sgpr_seq_rows_above(h, src, r, m, ld, ctx, None, row0, 10, flags, L, thr, rows, cols, vals, dirs, cap,
                                       row_ptr, count, ws, ws_bytes, None)

    _above_checks(lib, call, lambda: fn(h, R, M, 7))
    assert call(ld=M - 1) == -1
    assert call(r=-1) == -1 and call(m=-1) == -1
    # workspace queries answer 0 for invalid arguments and for empty calls
    assert fn(None, R, M, 7) == 0 and fn(h, R, M, -1) == 0 and fn(h, R, M, R + 1) == 0 and fn(h, -1, M, 0) == 0
    assert fn(h, R, M, R) == 0 and fn(h, 0, M, 0) == 0 and fn(h, R, 0, 0) == 0


def test_score_seq_above_argument_checks_touch_no_device(lib):
    keep, h = _zeroed_handle()
    fn = lib.sgpr_score_seq_above_workspace_bytes
    need = fn(h, R, M, 7, 8, FWD | REV)

    def call(h=h, src=P, colsrc=P, r=R, m=M, ctx=7, flags=FWD | REV, L=8, thr=0.5, rows=P, cols=P, vals=P, dirs=P, cap=10,
             row_ptr=P, count=P, ws=P, ws_bytes=need, row0=0):
        return lib.sgpr_score_seq_above(h, src, r, colsrc, m, ctx, None, row0, 10, flags, L, thr, rows, cols, vals, dirs,
                                        cap, row_ptr, count, ws, ws_bytes, None)

    _above_checks(lib, call, lambda: fn(h, R, M, 7, 8, FWD | REV))
    assert call(colsrc=None) == -1
    assert call(r=-1) == -1 and call(m=-1) == -1
    assert fn(None, R, M, 7, 8, FWD) == 0
    for L in (0, 33, -2):
        assert fn(h, R, M, 7, L, FWD) == 0
    for ctx in (-1, R + 1):
        assert fn(h, R, M, ctx, 8, FWD) == 0
    for flags in (0, CAUSAL, FWD | 8, -1):
        assert fn(h, R, M, 7, 8, flags) == 0
    assert fn(h, R, M, R, 8, FWD) == 0 and fn(h, 0, M, 0, 8, FWD) == 0 and fn(h, R, 0, 0, 8, FWD) == 0
    assert fn(h, R, M, 7, 8, FWD | REV | CAUSAL) == need == fn(h, R, M, 7, 8, REV)     # no dir block either way


def _eval_checks(lib, call):
    assert call(h=None) == -1
    assert call(src=None) == -1 and b"NULL" in lib.sgpr_last_error()
    assert call(colsrc=None) == -1
    assert call(pose=None, gt=None) == -1 and b"ground truth" in lib.sgpr_last_error()
    assert call(pose=None, gt=P, ldg=M - 1) == -1
    for L in (0, 33, -1):
        assert call(L=L) == -1 and b"sequence length" in lib.sgpr_last_error()
    for ctx in (-1, R + 1):
        assert call(ctx=ctx) == -1 and b"ctx" in lib.sgpr_last_error()
    assert call(flags=0) == -1 and b"direction" in lib.sgpr_last_error()
    assert call(flags=FWD | CAUSAL) == -1 and b"flag" in lib.sgpr_last_error()
    assert call(flags=FWD | 8) == -1 and call(flags=-1) == -1
    assert call(row0=0x7fffffff - 50) == -1 and b"row0" in lib.sgpr_last_error()
    assert call(out=None) == -1


def test_score_seq_positives_argument_checks_touch_no_device(lib):
    keep, h = _zeroed_handle()
    fn = lib.sgpr_score_seq_positives_workspace_bytes
    need = fn(h, R, M, 7, 8, FWD | REV)
    assert need > 0

    def call(h=h, src=P, colsrc=P, r=R, m=M, ctx=7, L=8, flags=FWD | REV, row0=0, pose=P, gt=None, ldg=M, dest=P, cap=10,
             out=P, ws=P, ws_bytes=need):
        return lib.sgpr_score_seq_positives(h, src, r, colsrc, m, ctx, L, flags, row0, pose, 3.0, 20.0, gt, ldg, dest, cap,
                                            out, ws, ws_bytes, None)

    _eval_checks(lib, call)
    assert call(cap=-1) == -1 and call(dest=None) == -1
    assert call(ws_bytes=need - 1) == -7 and call(ws=None) == -7
    assert fn(None, R, M, 7, 8, FWD) == 0 and fn(h, R, M, 7, 0, FWD) == 0 and fn(h, R, M, R + 1, 8, FWD) == 0
    assert fn(h, R, M, 7, 8, 0) == 0 and fn(h, R, M, 7, 8, FWD | CAUSAL) == 0 and fn(h, R, M, 7, 8, FWD | 8) == 0
    assert fn(h, R, M, R, 8, FWD) == 0 and fn(h, R, 0, 0, 8, FWD) == 0


def test_score_seq_threshold_counts_argument_checks_touch_no_device(lib):
    keep, h = _zeroed_handle()
    fn = lib.sgpr_score_seq_threshold_counts_workspace_bytes
    T = 100
    need = fn(h, R, M, 7, 8, FWD | REV, T)
    assert need > 0

    def call(h=h, src=P, colsrc=P, r=R, m=M, ctx=7, L=8, flags=FWD | REV, row0=0, pose=P, gt=None, ldg=M, thr=P, t=T,
             rank=None, gpt=0, at_least=None, out=P, ws=P, ws_bytes=need):
        return lib.sgpr_score_seq_threshold_counts(h, src, r, colsrc, m, ctx, L, flags, row0, pose, 3.0, 20.0, gt, ldg, thr,
                                                   t, rank, gpt, at_least, out, ws, ws_bytes, None)

    _eval_checks(lib, call)
    assert call(t=2048) == -1 and b"thresholds" in lib.sgpr_last_error()      # T beyond the limit
    assert call(t=-1) == -1 and call(thr=None) == -1
    assert call(rank=P, gpt=1, at_least=P, t=0, thr=None) == -1 and b"ranking" in lib.sgpr_last_error()
    assert call(rank=P, gpt=0, at_least=P) == -1 and call(rank=P, gpt=1, at_least=None) == -1
    assert call(ws_bytes=need - 1) == -7 and call(ws=None) == -7
    assert fn(h, R, M, 7, 8, FWD, 2048) == 0 and fn(h, R, M, 7, 8, FWD, -1) == 0 and fn(None, R, M, 7, 8, FWD, T) == 0
    assert fn(h, R, M, 7, 33, FWD, T) == 0 and fn(h, R, M, -1, 8, FWD, T) == 0 and fn(h, R, M, 7, 8, CAUSAL, T) == 0
    assert fn(h, R, M, R, 8, FWD, T) == 0
    # T enters through the counting slabs alone, one per CU (every block's counts fold straight into d_out)
    assert fn(h, R, M, 7, 8, FWD, 2047) == need                                # (a zeroed handle has no CU)
    cus = ctypes.create_string_buffer(1 << 16)
    struct.pack_into("ii", cus, 0, 0, 256)                                     # sgpr_handle: device, num_cus
    hc = ctypes.cast(cus, ctypes.c_void_p)

    def slabs(t):
        return (256 * ((((t + 2) & ~1) + 4) * 4) + 255) & ~255
    assert fn(hc, R, M, 7, 8, FWD, 2047) - fn(hc, R, M, 7, 8, FWD, T) == slabs(2047) - slabs(T)


@pytest.mark.parametrize("case", [(M_A, RB_A + 1, 8), (262144, 150, 32)], ids=["rb+1", "thin"])
def test_workspace_lies_below_the_list_forms(lib, case):
    """No Q block and no dir block: at least three quarters of one Q block below sgpr_score_seq_topk's at k = 1."""
    keep, h = _zeroed_handle()
    m, r, L = case
    rb = max(1, min(r, (64 << 20) // (4 * m) - (L - 1)))
    assert rb < r
    for flags in (FWD, REV | CAUSAL, FWD | REV):
        for ctx in (0, L - 1):
            above = lib.sgpr_score_seq_above_workspace_bytes(h, r, m, ctx, L, flags)
            topk = lib.sgpr_score_seq_topk_workspace_bytes(h, r, m, ctx, L, 1, flags)
            assert 0 < above < topk
            assert topk - above >= 0.75 * rb * m * 4, (case, flags, ctx, topk - above)
            # never grows with R * M: ten times the rows add the row pointer's 8 bytes per row and little else
            more = lib.sgpr_score_seq_above_workspace_bytes(h, 10 * r, m, ctx, L, flags)
            assert more - above <= 9 * r * 8 + (1 << 16)


def test_workspace_does_not_grow_with_the_matrix(lib):
    keep, h = _zeroed_handle()
    for L in (1, 8, 32):
        big = lib.sgpr_score_seq_above_workspace_bytes(h, 300000, 300000, L - 1, L, FWD | REV)
        assert 0 < big < (64 << 20) + (64 << 20) // 16 + 100 * 300000 + (32 << 20)
        for fn, extra in ((lib.sgpr_score_seq_positives_workspace_bytes, ()),
                          (lib.sgpr_score_seq_threshold_counts_workspace_bytes, (2047,))):
            ws = fn(h, 100000, 100000, 0, L, FWD | REV, *extra)
            ws2 = fn(h, 200000, 100000, 0, L, FWD | REV, *extra)
            assert 0 < ws < (160 << 20) and ws2 - ws < (1 << 20)      # a score block and a Q block, plus linear terms


def test_empty_calls_need_no_workspace(lib):
    """ctx == R, R == 0 and M == 0 are valid calls whose results (count 0, an all-zero row pointer) the device writes:
    the calls themselves run in tests/test_gpu_seq_above.py.  Here: they ask for no workspace."""
    keep, h = _zeroed_handle()
    assert lib.sgpr_score_seq_above_workspace_bytes(h, R, M, R, 8, FWD) == 0
    assert lib.sgpr_seq_rows_above_workspace_bytes(h, 0, M, 0) == 0
    assert lib.sgpr_score_seq_positives_workspace_bytes(h, R, 0, 3, 8, REV) == 0
    assert lib.sgpr_score_seq_threshold_counts_workspace_bytes(h, 0, 0, 0, 1, FWD, 0) == 0


# ------------------------------------------------------------------------------------------------- the reference
def test_reference_order_eligibility_and_row_pointer():
    rng = np.random.default_rng(3)
    s = rng.random((9, 13), dtype=np.float32)
    s[4, 5] = np.nan
    q, d = seq_ref.seq_filter(s, 3, 2, True, True)
    rows, cols, vals, dirs, row_ptr = seq_above_ref.seq_above(s, 3, -np.inf, ctx=2, forward=True, reverse=True, window=1,
                                                              row0=1)
    ok = seq_above_ref.eligible(9, 13, 2, 1, 1)
    assert ok.shape == (7, 13) and not ok[0, 2:5].any() and ok[0, 1] and ok[0, 5]      # row 2 is frame 3: columns 2..4 cut
    assert rows.size == int((ok & ~np.isnan(q)).sum()) == row_ptr[-1]                   # -inf: every non-NaN eligible pair
    assert (np.diff(rows.astype(np.int64) * 13 + cols) > 0).all()                       # row-major, ascending
    assert np.array_equal(vals.view(np.uint32), q[rows, cols].view(np.uint32)) and np.array_equal(dirs, d[rows, cols])
    assert np.array_equal(np.bincount(rows, minlength=7), np.diff(row_ptr))
    causal = seq_above_ref.eligible(9, 13, 0, -1, 0, causal=True)
    assert np.array_equal(causal, np.tril(np.ones((9, 13), dtype=bool), -1))
    perm = np.array([5, 0, 12, 3, 3, 7, 1, 9, 2])
    sel = seq_above_ref.eligible(9, 13, 1, 0, 0, causal=True, row_self=perm)
    assert [int(x.sum()) for x in sel] == perm[1:].tolist()
    # >= and > differ at a value that occurs
    v = np.float32(np.sort(q[~np.isnan(q)])[q.size // 2])
    n_ge = seq_above_ref.seq_above(s, 3, v, ctx=2, forward=True, reverse=True)[0].size
    assert n_ge == int((q >= v).sum()) > int((q > v).sum())
    assert seq_above_ref.seq_above(s, 3, np.inf, ctx=2)[0].size == 0
    assert seq_above_ref.seq_above(s, 3, 0.5, ctx=9)[4].tolist() == [0]


# ------------------------------------------------------------------------------------------------- the planted case
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_revisits_by_threshold(seed):
    """400 x 400, window 50, rows at least 8 into each revisit (184 true pairs), threshold 0.7: single scans take
    thousands of pairs, the sequence-matched score (L = 8, both directions) nearly the planted ones alone."""
    s, col = seq_ref.planted(seed)
    keep = np.concatenate((np.arange(208, 300), np.arange(308, 400)))
    assert keep.size == 184

    def rates(rows, cols):
        sel = np.isin(rows, keep)
        rows, cols = rows[sel], cols[sel]
        true = int((cols == col[rows]).sum())
        return rows.size, true / max(rows.size, 1), true / keep.size

    n1, p1, r1 = rates(*seq_above_ref.seq_above(s, 1, 0.7, window=50)[:2])
    rows, cols, vals, dirs, _ = seq_above_ref.seq_above(s, 8, 0.7, forward=True, reverse=True, window=50)
    n8, p8, r8 = rates(rows, cols)
    print("seed", seed, "S >= 0.7:", n1, p1, r1, " Q >= 0.7:", n8, p8, r8)
    assert p1 <= 0.05 and n1 > 20 * n8
    assert p8 >= 0.70 and r8 >= 0.95
    planted = np.isin(rows, keep) & (cols == col[rows])
    assert not dirs[planted & (rows < 300)].any() and dirs[planted & (rows >= 300)].all()
