"""sgpr_session_filter / sgpr_score_session_topk on the GPU: the session filter against the NumPy reference
(tests/session_ref.py) bit for bit, the two one-session identities against sgpr_seq_path_filter / sgpr_score_path_topk /
sgpr_score_seq_topk, the pooled form against score_all_pairs -> session_filter -> topk_rows_large(window=-1) on the same
rectangle (one block and several, on every kind of handle, a row seam on the first row of the second block and one inside
its context rows), dirty workspaces, empty cases, the planted three-session world, the place database online (with
new_session() in the middle) against one offline call, SG.loop_closures, the place_db CLI and tools/session_bench.py."""
import numpy as np
import pytest
import torch

import seq_path_ref
import session_ref
from test_gpu_row_blocks import M_A, RB_A
from test_gpu_score_range import _any_shape, _wide_checkpoint
from test_gpu_seq import DIRECTIONS, LENGTHS, _equal, _flags, _pooled, _same_bits, _scores, _seq_rb
from test_gpu_seq_paths import _path_sets
from test_gpu_stateless import _check_all_patterns
from test_session_host import planted_figures

pytestmark = pytest.mark.gpu

TR, TC = 32, 256                  # session_kernel's tile (SEQ_TR, SEQ_TC of sgpr_seq.hip): output rows x columns


@pytest.fixture(scope="module")
def sd(ckpt_path):
    from oracle import sgpr_oracle
    return sgpr_oracle.load_checkpoint(ckpt_path)


@pytest.fixture(scope="module")
def eng(sd):
    from sg_pr_amd import engine
    e = engine.Engine(sd, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def _tab(values, limit):
    """a valid table from seam positions: clipped to 0..limit, sorted (a clipped duplicate is an empty session)"""
    return np.sort(np.clip(np.asarray([0] + list(values), dtype=np.int64), 0, limit)).astype(np.int32)


def _col_tables(m):
    """column seams at 255 | 256 | 257 (two seams one apart), at 1, at M - 1 and at M; one session"""
    return [None, _tab([255, 256, 257], m), _tab([1, m - 1, m], m), _tab([256], m), _tab([255], m), _tab([257, m, m], m)]


def _row_tables(r, ctx):
    """row seams at ctx, at ctx + 31 | 32 | 33 (either side of the 32-row tile's edge) and at R; one session"""
    return [None, _tab([ctx, ctx + 31, r], r), _tab([ctx + 32], r), _tab([ctx + 33, r, r], r),
            _tab([ctx, ctx + 31, ctx + 32, ctx + 33, r], r), _tab([1, 2], r)]


# ------------------------------------------------------------------------------------------------- 1. the filter
FILTER_SHAPES = [(1, 1, 0, 0), (5, 7, 0, 0), (37, 131, 0, 0), (70, 300, 3, 5),
                 (TR + 1, TC - 1, 0, 0), (TR + 1, TC + 1, 0, 0), (TR + 1, 2 * TC + 3, 0, 0)]


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=["%dx%d" % s[:2] for s in FILTER_SHAPES])
def test_filter_equals_the_reference(eng, shape):
    r, m, pad_in, pad_out = shape
    host = _scores(r, m, 5 * r + m, ld=m + pad_in)
    dev = torch.from_numpy(host).cuda()[:, :m]               # ld = m + pad_in: read in place
    assert dev.stride(0) == m + pad_in or r == 1
    rng = np.random.default_rng(r * m)
    explicit = rng.integers(-2, m + 3, size=r).astype(np.int32)          # row frames below 0 and at or past M too
    selfs = [dict(row0=0), dict(row0=7), dict(row0=m), dict(row_self=explicit)]
    n = 0
    excluded = seams = 0
    for L in LENGTHS:
        ctxs = sorted({0, min(1, r), min(L - 1, r), r - 1})
        for name, paths in _path_sets(L):
            for reverse in DIRECTIONS:
                for rep in range(2):                          # two settings per (L, path set, direction), rotating
                    ctx = ctxs[(n + rep) % len(ctxs)]
                    rt = _row_tables(r, ctx)[(n // 2 + 3 * rep) % 6]
                    ct = _col_tables(m)[(n + 1 + 2 * rep) % 6]
                    window = (-1, 0, 3)[(n // 3 + rep) % 3]
                    who = selfs[(n // 5 + rep) % 4]
                    table = None if (name == "unit" and n % 2) else paths      # no table: the unit diagonal
                    wq, wc = session_ref.session_filter(host[:, :m], table, L=L, ctx=ctx, row_starts=rt, col_starts=ct,
                                                        window=window, **who, **_flags(reverse))
                    ro = r - ctx
                    out = torch.full((ro, m + pad_out), 7.0, device="cuda")
                    ocode = torch.full((ro, m + pad_out), 99, dtype=torch.uint8, device="cuda")
                    q, c = eng.session_filter(dev, L, table, row_sessions=rt, col_sessions=ct, window=window, context=ctx,
                                              reverse=reverse, out=out[:, :m], out_code=ocode[:, :m], **who)
                    what = (shape, L, name, reverse, ctx, None if rt is None else rt.tolist(),
                            None if ct is None else ct.tolist(), window, sorted(who))
                    _same_bits(q.cpu().numpy(), wq, what)
                    assert np.array_equal(c.cpu().numpy(), wc), what
                    if pad_out:                               # nothing written past column m of an output row
                        assert (out[:, m:] == 7.0).all() and (ocode[:, m:] == 99).all(), what
                    if window >= 0:
                        excluded += int(session_ref.excluded(r, m, ct, window, who.get("row_self"), who.get("row0", 0))[ctx:].sum())
                    seams += (rt is not None) + (ct is not None)
                n += 1
    assert seams > 100 and (excluded > 0 or m == 1)
    q = eng.session_filter(dev, 3, None, col_sessions=_tab([1], m), window=0)      # without the code
    _same_bits(q.cpu().numpy(), session_ref.session_filter(host[:, :m], None, L=3, col_starts=_tab([1], m), window=0)[0],
               (shape, "no code"))
    assert eng.session_filter(dev, 3, None, context=r, row_sessions=[0, r]).shape == (0, m)


def test_filter_block_identity_on_the_device(eng):
    """window = -1: every (row session, column session) block is seq_path_filter run on that sub-matrix alone"""
    r, m = 70, 600
    rt, ct = _tab([1, 20, 20, 52], r), _tab([255, 256, 300, 300, 599, 600], m)
    dev = torch.from_numpy(_scores(r, m, 21)).cuda()
    for L, reverse in ((8, "both"), (32, False), (3, True)):
        paths = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
        for ctx in (0, 5):
            q, c = eng.session_filter(dev, L, paths, row_sessions=rt, col_sessions=ct, context=ctx, reverse=reverse,
                                      want_code=True)
            for ra, rb in zip(rt.tolist(), rt.tolist()[1:] + [r]):
                if rb <= max(ra, ctx):
                    continue
                for ca, cb in zip(ct.tolist(), ct.tolist()[1:] + [m]):
                    if cb <= ca:
                        continue
                    want = eng.seq_path_filter(dev[ra:rb, ca:cb], L, paths, context=max(ctx - ra, 0), reverse=reverse,
                                               want_code=True)
                    o = max(ra, ctx) - ctx
                    _equal((q[o:rb - ctx, ca:cb], c[o:rb - ctx, ca:cb]), want, (L, reverse, ctx, (ra, rb), (ca, cb)))


# ------------------------------------------------------------------------------------------------- 2. one session
def test_one_session_filter_is_the_path_filter(eng):
    dev = torch.from_numpy(_scores(70, 300, 5)).cuda()
    for L in LENGTHS:
        for name, paths in _path_sets(L)[:2]:
            for reverse in DIRECTIONS:
                for ctx in (0, L - 1):
                    want = eng.seq_path_filter(dev, L, paths, context=ctx, reverse=reverse, want_code=True)
                    for tables in (dict(), dict(row_sessions=[0], col_sessions=[0])):
                        got = eng.session_filter(dev, L, paths, context=ctx, reverse=reverse, want_code=True, **tables)
                        _equal(got, want, ("one session", L, name, reverse, ctx, sorted(tables)))
                    if name == "unit":
                        _equal(eng.session_filter(dev, L, None, context=ctx, reverse=reverse, want_code=True),
                               eng.seq_filter(dev, L, context=ctx, reverse=reverse, want_dir=True), ("no table", L, ctx))


def test_one_session_pooled_is_path_topk_and_seq_topk(eng):
    rows, cols = _pooled(300, 32, 3.0, 1), _pooled(517, 32, 3.0, 2)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(517)[:300].astype(np.int32))
    n = 0
    for L in (1, 8, 32):
        nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
        for k in (1, 17):
            for elig in (dict(window=-1), dict(window=50, causal=True), dict(window=10, row0=3),
                         dict(window=10, row_self=perm, causal=True)):
                reverse = DIRECTIONS[n % 3]
                tables = (dict(), dict(row_sessions=[0], col_sessions=[0]))[n % 2]
                n += 1
                kw = dict(k=k, context=L - 1, reverse=reverse, **elig)
                _equal(eng.score_session_topk(rows, cols, L, nine, **tables, **kw),
                       eng.score_path_topk(rows, cols, L, nine, radius=0, **kw), ("nine paths", L, kw))
                _equal(eng.score_session_topk(rows, cols, L, None, **tables, **kw), eng.score_seq_topk(rows, cols, L, **kw),
                       ("no table", L, kw))
                ws = dict(k=k, context=L - 1, reverse=reverse, causal=elig.get("causal", False))
                for n_paths in (nine.shape[0], 0):            # (no table counts as one path)
                    assert eng.score_session_topk_workspace_bytes(300, 517, L, n_paths, n_row_sessions=1,
                                                                  n_col_sessions=1, **ws) == \
                        eng.score_path_topk_workspace_bytes(300, 517, L, max(n_paths, 1), **ws)
    eng.check_status()


# ------------------------------------------------------------------------------------------------- 3. the pooled form
def _reference(e, rows, cols, L, paths, k, row_sessions=None, col_sessions=None, window=-1, row0=0, causal=False,
               row_self=None, context=0, reverse="both", score=None):
    """score_all_pairs -> session_filter -> topk_rows_large without a window on the same rectangle, codes gathered"""
    score = e.score_all_pairs(rows, cols) if score is None else score
    q, c = e.session_filter(score, L, paths, row_sessions=row_sessions, col_sessions=col_sessions, window=window,
                            row0=row0, row_self=row_self, context=context, reverse=reverse, want_code=True)
    rs = None if row_self is None else row_self[context:]
    v, i = e.topk_rows_large(q, k=k, row0=row0 + context, window=-1, causal=causal, row_self=rs)
    codes = torch.where(i >= 0, c.gather(1, i.clamp(min=0).long()), torch.zeros_like(i, dtype=torch.uint8))
    return v, i, codes


@pytest.mark.parametrize("shape", [(37, 131), (300, 517)])
def test_pooled_equals_matrix_filter_selection(eng, shape):
    r, m = shape
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    host = score.cpu().numpy()
    perm = torch.from_numpy(np.random.default_rng(r).permutation(m)[:r].astype(np.int32))
    modes = [dict(window=-1), dict(window=0), dict(window=50, causal=True), dict(window=10, row_self=perm),
             dict(window=10, causal=True, row_self=perm), dict(window=50, row0=m - r)]
    rts = [None, _tab([r // 3, r // 3 + 1, r - 1], r), _tab([3, r // 2, r], r)]
    cts = [_tab([m // 2], m), _tab([1, m // 3, m // 3, m - 1, m], m), None, _tab([256, 257], m)]
    n = 0
    for L in (1, 2, 8, 32):
        sets = _path_sets(L)
        for ctx in sorted({0, 3, L - 1}):
            for j, mode in enumerate(modes):
                k = (1, 17, 4, m + 5)[(j + n) % 4]
                reverse = DIRECTIONS[(j + n // 3) % 3]
                name, paths = sets[(j + n) % len(sets)]
                kw = dict(k=k, context=ctx, reverse=reverse, row_sessions=rts[(j + n) % 3], col_sessions=cts[(j + n // 2) % 4],
                          **mode)
                got = eng.score_session_topk(rows, cols, L, paths, **kw)
                _equal(got, _reference(eng, rows, cols, L, paths, score=score, **kw), (shape, L, name, kw))
                assert got[0].shape == (r - ctx, k)
                if r < 100 and j % 2 == 0:                    # ... and the NumPy reference end to end
                    rs = mode.get("row_self")
                    rs = None if rs is None else rs.numpy()
                    wq, wc = session_ref.session_filter(host, paths, ctx=ctx, row_starts=kw["row_sessions"],
                                                        col_starts=kw["col_sessions"], window=mode["window"], row_self=rs,
                                                        row0=mode.get("row0", 0), **_flags(reverse))
                    wv, wi = session_ref.topk(wq, k, None if rs is None else rs[ctx:], mode.get("row0", 0) + ctx,
                                              mode.get("causal", False))
                    _same_bits(got[0].cpu().numpy(), wv, ("reference", shape, L, name, kw))
                    assert np.array_equal(got[1].cpu().numpy(), wi), ("reference", shape, L, name, kw)
                    assert np.array_equal(got[2].cpu().numpy(), np.where(wi >= 0, np.take_along_axis(wc, np.maximum(wi, 0), 1), 0))
            n += 1
    eng.check_status()


def _block_tables(r, m, L):
    """a row seam on the first row of the second block and another inside its context rows; three column sessions"""
    rb = _seq_rb(r, m, L)
    assert rb < r and L >= 4                                   # more than one block runs
    return _tab([rb - (L - 1) // 2, rb], r), _tab([m // 3, m // 3 + 300], m)


def test_several_blocks_tuned_handle(eng):
    m, r, L = M_A, RB_A + 1, 8
    rt, ct = _block_tables(r, m, L)
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    assert eng.score_session_topk_workspace_bytes(r, m, L, 9, k=17, reverse=True, n_row_sessions=3, n_col_sessions=3) == \
        eng.score_path_topk_workspace_bytes(r, m, L, 9, k=17, reverse=True)
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    score = eng.score_all_pairs(rows, cols)
    perm = torch.from_numpy(np.random.default_rng(r).integers(0, m, size=r).astype(np.int32))
    for kw in (dict(k=17, window=50, context=L - 1), dict(k=1, window=5, row0=7, causal=True, reverse=True),
               dict(k=1, window=10, causal=True, row_self=perm, reverse=False, context=3)):
        got = eng.score_session_topk(rows, cols, L, nine, row_sessions=rt, col_sessions=ct, **kw)
        _equal(got, _reference(eng, rows, cols, L, nine, score=score, row_sessions=rt, col_sessions=ct, **kw),
               ("tuned, blocks", kw))
    eng.check_status()


def test_several_blocks_thin(eng):
    m, r, L = 262144, 70, 32
    assert _seq_rb(r, m, L) == 33 < r                          # the context nearly fills a block: 31 + 33 rows of 1 MB
    rt, ct = _block_tables(r, m, L)
    paths = _path_sets(L)[2][1]                                # the jump of 64: the widest halo, the deepest LDS tile
    rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
    kw = dict(k=17, window=50, context=L - 1, row_sessions=rt, col_sessions=ct)
    _equal(eng.score_session_topk(rows, cols, L, paths, **kw), _reference(eng, rows, cols, L, paths, **kw), ("thin", kw))
    eng.check_status()


def test_several_blocks_wide_checkpoint(sd):
    from sg_pr_amd import engine
    m, r, L = M_A, RB_A + 1, 8
    rt, ct = _block_tables(r, m, L)
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    wide = engine.Engine(_wide_checkpoint(sd), device=0)
    try:
        assert not wide.uses_f16_planes()
        rows, cols = _pooled(r, 32, 3.0, r), _pooled(m, 32, 3.0, m)
        kw = dict(k=17, window=50, context=L - 1, row_sessions=rt, col_sessions=ct)
        _equal(wide.score_session_topk(rows, cols, L, nine, **kw), _reference(wide, rows, cols, L, nine, **kw),
               ("wide checkpoint", kw))
        wide.check_status()
    finally:
        wide.close()


def test_several_blocks_any_shape():
    m, r, L = M_A, RB_A + 1, 8
    rt, ct = _block_tables(r, m, L)
    nine = seq_path_ref.seq_paths(L, seq_path_ref.SLOPES)
    any_eng = _any_shape(_any_shape())
    try:
        assert any_eng.any_shape
        rows, cols = _pooled(r, 48, 1.0, r + 1), _pooled(m, 48, 1.0, m + 1)
        kw = dict(k=17, window=50, causal=True, context=2, row_sessions=rt, col_sessions=ct)
        _equal(any_eng.score_session_topk(rows, cols, L, nine, **kw), _reference(any_eng, rows, cols, L, nine, **kw),
               ("any-shape", kw))
        any_eng.check_status()
    finally:
        any_eng.close()


# ------------------------------------------------------------------------------------------------- 4. other cases
def test_dirty_workspaces(eng):
    rows, cols = _pooled(300, 32, 3.0, 5), _pooled(4541, 32, 3.0, 6)
    score = torch.from_numpy(_scores(300, 4541, 13)).cuda()
    nine = seq_path_ref.seq_paths(8, seq_path_ref.SLOPES)
    rt, ct = _tab([7, 100, 101], 300), _tab([1500, 3000], 4541)
    base = _check_all_patterns(eng, lambda: eng.score_session_topk(rows, cols, 8, nine, row_sessions=rt, col_sessions=ct,
                                                                   k=100, window=50, causal=True, context=7),
                               "score_session_topk")
    assert base[0].shape == (293, 100)
    _check_all_patterns(eng, lambda: eng.score_session_topk(rows, cols, 8, None, col_sessions=ct, k=3, window=50,
                                                            reverse=True), "score_session_topk, one direction, no table")
    _check_all_patterns(eng, lambda: eng.session_filter(score, 8, nine, row_sessions=rt, col_sessions=ct, window=50,
                                                        reverse="both", want_code=True), "session_filter")


def test_empty_cases(eng):
    rows, cols = _pooled(37, 32, 3.0, 8), _pooled(131, 32, 3.0, 9)
    nine = seq_path_ref.seq_paths(8, seq_path_ref.SLOPES)
    v, i, c = eng.score_session_topk(rows, cols, 8, nine, k=3, context=37, row_sessions=[0, 37], col_sessions=[0, 131])
    assert v.shape == (0, 3) and i.shape == (0, 3) and c.shape == (0, 3)
    v, i, c = eng.score_session_topk(rows, cols[:0], 8, nine, k=3, context=2, reverse=True, col_sessions=[0, 0], window=5)
    assert v.shape == (35, 3) and (v == -float("inf")).all() and (i == -1).all() and not c.any()
    v, i, c = eng.score_session_topk(rows[:0], cols, 8, None, k=3)
    assert v.shape == (0, 3)
    # a window that covers a whole one-session map: every end point excluded, padding lists
    v, i, c = eng.score_session_topk(rows, cols, 8, nine, k=3, window=200)
    assert (v == -float("inf")).all() and (i == -1).all() and not c.any()
    # ... and with the columns in another session than every row frame nothing is excluded
    v, i, c = eng.score_session_topk(rows, cols, 8, nine, k=3, window=200, row0=131, col_sessions=[0, 131])
    assert (i >= 0).all()
    assert eng.session_filter(torch.zeros(0, 5, device="cuda"), 3, None).shape == (0, 5)
    assert eng.session_filter(torch.zeros(4, 0, device="cuda"), 3, None, col_sessions=[0, 0]).shape == (4, 0)
    from sg_pr_amd.engine import SgprError
    for bad in (dict(col_sessions=[0, 132]), dict(row_sessions=[1]), dict(col_sessions=[0, 5, 4]),
                dict(row_sessions=np.zeros(65, dtype=np.int32))):
        with pytest.raises(SgprError):
            eng.score_session_topk(rows, cols, 8, nine, **bad)
    eng.check_status()


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_planted_world_on_the_device(eng, seed):
    """the planted gates of tests/test_session_host.py on the device's lists: they are the reference's figures"""
    L, window = 8, 50
    s, col = session_ref.planted(seed)
    dev = torch.from_numpy(s).cuda()
    groups = session_ref.planted_groups(L, window)
    today = eng.topk_rows_large(eng.seq_filter(dev, L, reverse="both"), k=1, window=window)[1][:, 0].cpu().numpy()
    q = eng.session_filter(dev, L, None, row_sessions=session_ref.WORLD_STARTS, col_sessions=session_ref.WORLD_STARTS,
                           window=window, reverse="both")
    sess = eng.topk_rows_large(q, k=1)[1][:, 0].cpu().numpy()
    got = ([session_ref.recall(today, col, g) for g in groups], [session_ref.recall(sess, col, g) for g in groups])
    print("seed", seed, "today (B head, C head, rest):", got[0], "session form:", got[1])
    assert got[0][0] == 0.0 and got[1][0] >= 0.6 and got[1][1] >= 0.7 and got[0][1] <= 0.65
    assert got == planted_figures(seed, L, window)


# ------------------------------------------------------------------------------------------------- 5. online = offline
def test_place_database_online_equals_offline(model):
    """query_seq before every append (causal, L = 8, k = 4), new_session() called twice on the way, against one
    score_session_topk call over the whole map with the same tables; window >= the paths' largest offset, so no reverse
    sum of an eligible column of the current session reaches a member that is not stored yet."""
    from sg_pr_amd import engine
    from sg_pr_amd.place_db import PlaceDatabase
    n, L, k = 120, 8, 4
    seams = (50, 53)                                           # the third session starts three scans into the second
    paths = engine.seq_paths(L, seq_path_ref.SLOPES)
    window = int(paths.max())
    pooled = _pooled(n, 32, 3.0, 77)
    e = model.engine()
    for slopes, table in ((seq_path_ref.SLOPES, paths), (None, None)):
        db = PlaceDatabase(model, capacity=4)
        got, single = [], []
        for t in range(n):
            if t in seams:
                db.new_session()
            got.append(db.query_seq(None, None, L, k=k, window=window, causal=True, pooled=pooled[t:t + 1], slopes=slopes))
            db.append_pooled(pooled[t:t + 1])
            single.append(db.query_ids([t], k=k, window=window, causal=True))
        starts = db.session_starts
        assert starts.tolist() == [0, 50, 53]
        online = tuple(torch.cat([g[j] for g in got]) for j in range(3))
        offline = e.score_session_topk(pooled, pooled, L, table, row_sessions=starts, col_sessions=starts, k=k,
                                       window=window, causal=True)
        _equal(online, offline, ("online / offline", slopes))
        # the first scans of a session see the end of the one before: nothing of another session is window-excluded
        assert (offline[1][50] >= 0).all()
        assert (offline[1][:window + 1] == -1).all()
        # L = 1: S under the session window
        flat = e.score_session_topk(pooled, pooled, 1, None, col_sessions=starts, k=k, window=window, causal=True,
                                    reverse=False)
        _equal(tuple(torch.cat([g[j] for g in single]) for j in range(2)), flat[:2], "query_ids, one at a time")
        _equal(db.query_ids(torch.arange(n), k=k, window=window), e.score_session_topk(
            pooled, pooled, 1, None, col_sessions=starts, k=k, window=window, reverse=False)[:2], "query_ids")
        # a run of members across both seams
        run = db.query_ids_seq(40, 30, L, k=k, window=window, slopes=slopes)
        want = e.score_session_topk(pooled, pooled, L, table, row_sessions=starts, col_sessions=starts, k=k, window=window)
        _equal(run, tuple(w[40:70] for w in want), ("query_ids_seq", slopes))
    with pytest.raises(NotImplementedError):
        db.query_ids_seq(40, 30, L, distinct=5)
    # a database that never called new_session(): exactly today's calls
    one = PlaceDatabase(model, capacity=4)
    one.append_pooled(pooled)
    _equal(one.query_ids_seq(40, 30, L, k=k, window=window), tuple(
        w[40:70] for w in e.score_seq_topk(pooled, pooled, L, k=k, window=window)), "no session call")
    e.check_status()


def test_loop_closures_session_tables(model):
    e = model.engine()
    pooled = _pooled(150, 32, 3.0, 78)
    starts = [0, 60, 100]
    for kw in (dict(k=4, window=16), dict(k=4, window=16, seq_len=8), dict(k=3, window=16, seq_len=8, distinct=5)):
        _equal(model.loop_closures(pooled, pooled, row_sessions=None, col_sessions=None, **kw),
               model.loop_closures(pooled, pooled, **kw), ("no tables", kw))
    _equal(model.loop_closures(pooled, pooled, k=4, window=16, seq_len=8, row_sessions=starts, col_sessions=starts),
           e.score_session_topk(pooled, pooled, 8, None, row_sessions=starts, col_sessions=starts, k=4, window=16), "tables")
    paths = seq_path_ref.seq_paths(8, ["1", "1/2", "2"])
    _equal(model.loop_closures(pooled, pooled, k=4, window=16, seq_len=8, seq_slopes=["1", "1/2", "2"], causal=True,
                               col_sessions=starts, seq_reverse=True),
           e.score_session_topk(pooled, pooled, 8, paths, col_sessions=starts, k=4, window=16, causal=True, reverse=True),
           "tables, slopes")
    _equal(model.loop_closures(pooled, pooled, k=2, window=16, col_sessions=starts),
           e.score_session_topk(pooled, pooled, 1, None, col_sessions=starts, k=2, window=16), "tables, L = 1")
    with pytest.raises(ValueError):
        model.loop_closures(pooled, pooled, k=2, window=16, distinct=5, col_sessions=starts)


# ------------------------------------------------------------------------------------------------- 6. the tools
def test_place_db_cli_sessions(model, tmp_path, ckpt_path, capsys):
    import os
    from sg_pr_amd import graph_store, place_db, synth
    n = 120
    centers, labels, _, poses = synth.world_sequence(n, 100, seed=4)
    seq = graph_store.PackedSequence(centers, labels, poses, ["%d.json" % j for j in range(n)])
    os.makedirs(tmp_path / "eva")
    seq.save(str(tmp_path / "eva" / "07_packed.npz"))
    cfg = tmp_path / "config.yml"
    cfg.write_text("""
common: {model: "%s", cuda: "0", batch_size: 128, p_thresh: 3, graph_pairs_dir: "%s", pair_list_dir: '%s'}
arch: {keep_node: 1, filters_1: 64, filters_2: 64, filters_3: 32, tensor_neurons: 16, bottle_neck_neurons: 16, K: 10}
train: {epochs: 500, train_sequences: ['00'], eval_sequences: ["08"], dropout: 0, learning_rate: 0.001,
        weight_decay: 0.0005, gpu: 0, logdir: "./logs_k10", node_num: 100}
eva_batch: {sequences: ["07"], output_path: "%s", show: False}
eva_pair: {pair_file: ["a.json", "b.json"]}
""" % (ckpt_path, tmp_path / "graphs", tmp_path, tmp_path / "eva"))
    eng = model.engine()
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    starts = [0, 40, 80]
    for extra, L, paths in ((["--seq-len", "8"], 8, None), ([], 1, None),
                            (["--seq-len", "8", "--seq-slopes", "1,1/2,2"], 8, seq_path_ref.seq_paths(8, ["1", "1/2", "2"]))):
        place_db.main([str(cfg), "--k", "3", "--window", "14", "--sessions", "3"] + extra)
        lines = [l for l in capsys.readouterr().out.splitlines() if " sessions 3 " in l]
        assert len(lines) == 2 and "all rows" in lines[0] and "head rows (28)" in lines[1], lines
        assert all("recall@1" in l and "recall@3" in l and "one trajectory" in l for l in lines)
        z = np.load(tmp_path / "eva" / "07_sessions.npz")
        assert sorted(z.files) == sorted(["frame", "indices", "scores", "codes", "session_starts", "recall", "recall_head",
                                          "recall_one_trajectory", "recall_head_one_trajectory", "head_rows"] +
                                         (["seq_len"] if L > 1 else []))
        assert z["session_starts"].tolist() == starts and int(z["head_rows"]) == 28
        v, i, c = eng.score_session_topk(pooled, pooled, L, paths, row_sessions=starts, col_sessions=starts, k=3, window=14,
                                         reverse="both" if L > 1 else False)
        assert np.array_equal(z["indices"], i.cpu().numpy())
        assert np.array_equal(z["scores"].view(np.uint32), v.cpu().numpy().view(np.uint32))
        if L > 1:
            assert np.array_equal(z["codes"], c.cpu().numpy())
        assert "recall@1 %.4f (one trajectory %.4f)" % (z["recall"][0], z["recall_one_trajectory"][0]) in lines[0]
        assert "recall@1 %.4f (one trajectory %.4f)" % (z["recall_head"][0], z["recall_head_one_trajectory"][0]) in lines[1]
    place_db.main([str(cfg), "--k", "3", "--window", "14", "--seq-len", "8"])       # without the flag: as before
    assert sorted(np.load(tmp_path / "eva" / "07_topk.npz").files) == ["dirs", "frame", "indices", "recall", "scores", "seq_len"]
    for bad in (["--sessions", "1"], ["--sessions", "65"], ["--sessions", "3", "--distinct", "5"]):
        with pytest.raises(SystemExit):
            place_db.main([str(cfg)] + bad)


def test_session_bench_tool(capsys):
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import session_bench
    recs = session_bench.main(["--tiny"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert lines == recs
    calls = [r for r in recs if "path_ms" in r]
    assert {(r["seq_len"], r["k"], r["paths"]) for r in calls} == {(L, k, p) for L in (8, 16) for k in (1, 16) for p in (1, 9)}
    assert all(r["one_session_lists_equal"] and r["path_ms"] > 0 and r["session1_ms"] > 0 and r["session4_ms"] > 0
               and r["session1_over_path"] > 0 and r["path_peak_mb"] > 0
               and abs(r["session1_peak_mb"] - r["path_peak_mb"]) <= 1.0 for r in calls)
    recall = [r for r in recs if "recall1_all" in r]
    assert {(r["seq_len"], r["k"]) for r in recall} == {(L, k) for L in (8, 16) for k in (1, 16)}
    assert all(r["sessions"] == 4 and r["head_rows"] == 150 and 0.0 <= r["recall1_head"] <= 1.0 for r in recall)
