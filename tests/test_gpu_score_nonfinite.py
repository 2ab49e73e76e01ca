"""Non-finite pooled vectors through every scoring entry point and every consumer: NaN in, NaN out.

A NaN pooled vector is the library's own error marker (include/sgpr.h: a graph that breaks its node promise), and top-k,
range retrieval, mining, the threshold counters and the sequence filter all document "a NaN score never qualifies".  The
link between the two - a NaN vector gives a NaN score - is what this file holds every kernel to, against the float64 tail
of tests/score_ref.py under the rule of tests/nonfinite_ref.py (host-tested in tests/test_nonfinite_host.py):
  a NaN anywhere in a graph's vector: every pair of that graph is NaN;
  a +-inf: NaN, or within the bar of the reference where that is not NaN (one-sided: the order of infinite terms is free);
  two finite graphs: within the bar, whatever else shares their launch.
Plants (nonfinite_ref.plants): whole graphs of 0x7fc00000 (the embed kernels' marker) and 0xffc00000 (which a signed-integer
ReLU would turn into 0), written through an integer view; one NaN element at the first, the two middle and the last index
of four rows / four columns, the last row and column (a partial tile of 37 x 131) among them; one +inf, one -inf, both in
one row, a row of +inf; the square case rows is cols.  Every handle kind of test_gpu_score_range; the control is that
file's _check on the same inputs without a plant.

The bar is test_gpu_score_range's BAR for every entry point: a launch that meets a non-finite operand takes the exact fp32
per-pair path on every handle (sgpr_score.hip range_max / ap_mode; the any-shape tail's gate), which is the arithmetic BAR
was set for; BAR_BF16 and EPS_COND stay with the control (the three-plane path, large head terms).  The bitwise contracts
between entry points are _check's, with NaN positions comparing equal.

Before the kernels kept NaN (the fmaxf ReLU of the exact paths: fmaxf(NaN, 0) = 0; no NaN marker in the tuned tail's
range partials; no per-pair path behind the three-plane tail) every test of this file failed on an MI355X, on all five
handle kinds alike: every pair of a NaN graph, in all five NaN plants (both sign bits, whole vectors and single elements,
the square case) and through score_pairs, score_pair_list, score_all_pairs and score_all_pairs_multi, came out as ONE
finite value, 0.577959 on the shipped checkpoint (0.542533 on the any-shape one) = sigmoid(fc2 . relu(fc1_b) + fc2_b):
the fmaxf paths and both matrix-core tails zero a NaN H alike.  The consumers then listed the NaN row's columns
(score_topk index 0 for the NaN row, score_above 40 pairs of it).  The four +-inf plants passed before and after.
The record of that run is profiles/nonfinite_before_after.txt."""
import numpy as np
import pytest
import torch

import nonfinite_ref as nf
import score_ref
import seq_ref
from test_gpu_score_range import BAR, HANDLES, N_PAIRS, _any_shape, _check, _engine, _inputs
from test_gpu_topk import _reference as _topk_reference

pytestmark = pytest.mark.gpu

IDS = [h[0] for h in HANDLES]
INF = float("inf")


def _same(a, b):
    """torch.equal with NaN positions comparing equal"""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _base_sd(kind, oracle_sd):
    return _any_shape() if kind == "any" else oracle_sd


def _dev(a):
    return torch.from_numpy(a).cuda()               # (a copy of the bytes: the planted bit patterns arrive as they are)


def _bad_graphs(a):
    return np.nonzero(~np.isfinite(a).all(axis=1))[0]


def _check_plant(eng, sd, kind, a_np, b_np, square, what):
    """Every entry point on one planted input against the rule, and the contracts between them -> list of failures."""
    cls, ref = nf.classes(sd, a_np, b_np)
    tol = np.full(cls.shape, BAR)
    r, m = cls.shape
    rows = _dev(a_np)
    cols = rows if square else _dev(b_np)
    fails = []

    def rule(name, got, pick=None):
        g = got.cpu().numpy()
        c, s, t = (cls, ref["score"], tol) if pick is None else (cls[pick], ref["score"][pick], tol[pick])
        bad = nf.violations(g, c, {"score": s}, t)
        if bad.any():
            lost = bad & (c == nf.MUST_NAN)
            fin = g[lost]
            fails.append("%s: %s: %d of %d pairs break the rule, %d of them a NaN that came out finite (%s)"
                         % (what, name, int(bad.sum()), bad.size, int(lost.sum()),
                            "values %.6g .. %.6g" % (fin.min(), fin.max()) if fin.size else "none"))

    def contract(name, ok):
        if not ok:
            fails.append("%s: contract: %s" % (what, name))

    ii, jj = torch.meshgrid(torch.arange(r, dtype=torch.int32), torch.arange(m, dtype=torch.int32), indexing="ij")
    sp = eng.score_pairs(rows, cols, ii.reshape(-1), jj.reshape(-1)).view(r, m)
    rule("score_pairs", sp)
    spd = eng.score_pairs(rows.repeat_interleave(m, 0), cols.repeat(r, 1)).view(r, m)        # without index arrays
    contract("score_pairs with and without index arrays", _same(spd, sp))
    mat = eng.score_all_pairs(rows, cols)
    rule("score_all_pairs", mat)
    g = np.random.default_rng(r * 1000 + m)
    i1, i2 = g.integers(0, r, N_PAIRS), g.integers(0, m, N_PAIRS)
    i1[:3], i2[:3] = 0, m - 1
    touched = cls[i1, i2] != nf.FINITE
    assert touched.sum() > 5 and (~touched).sum() > 1000           # the list holds planted and healthy pairs
    pl = eng.score_pair_list(rows, cols, eng.pair_plan(i1, i2, r, m))
    rule("score_pair_list", pl, (i1, i2))
    t1, t2 = _dev(i1), _dev(i2)
    if kind == "f16":
        contract("pair list == matrix entries", _same(pl, mat[t1, t2]))
    elif kind == "any":
        contract("pair list == score_pairs", _same(pl, sp[t1, t2]))
    else:       # wide-range tails: the list kernel's exact fp32 arithmetic - score_pairs' to rounding; with an infinite
        #         operand the two may meet the infinite terms in different orders: NaN and healthy pairs only
        k = torch.from_numpy(np.isin(cls[i1, i2], (nf.FINITE, nf.MUST_NAN))).cuda()
        a, b = pl[k], sp[t1, t2][k]
        contract("pair list NaN pattern == score_pairs'", bool((torch.isnan(a) == torch.isnan(b)).all()))
        d = (a - b)[~torch.isnan(a) & ~torch.isnan(b)]
        contract("pair list within 1e-6 of score_pairs", d.numel() == 0 or d.abs().max().item() <= 1e-6)
    # the jobs of _check: more than 8 ragged rectangles (two calls of the C entry point), an empty one, a padded output
    jobs = [(rows[:17], cols), (rows[:1], cols[:65]), (rows, cols[:1]), (rows[5:], cols[3:]), (rows[:0], cols),
            (rows[2:19], cols[:131]), (rows, cols, torch.empty(r, m + 7, device="cuda")[:, :m])]
    jobs = jobs + jobs[:4]
    got = eng.score_all_pairs_multi(jobs)
    for n, ((jr, jc, *_), g_) in enumerate(zip(jobs, got)):
        if g_.numel():
            contract("multi job %d == single" % n, _same(g_, eng.score_all_pairs(jr.contiguous(), jc.contiguous())))
    rule("score_all_pairs_multi (whole rectangle, padded output)", got[6])
    rule("score_all_pairs_multi (rows 5.., columns 3..)", got[3], (slice(5, None), slice(3, None)))
    for k in (1, 16):
        for causal in (False, True):
            v, ix = eng.score_topk(rows, cols, k=k, window=2, causal=causal)
            wv, wi = _topk_reference(mat, k, window=2, causal=causal)
            bad = ((v != wv) & ~(torch.isinf(v) & torch.isinf(wv))) | (ix != wi)
            contract("score_topk k %d causal %d == the matrix's stable sort" % (k, causal), not bad.any())
    return fails


@pytest.mark.parametrize("handle", HANDLES, ids=IDS)
def test_every_entry_point_on_every_plant(oracle_sd, handle):
    name, kind, mask = handle
    sd = _base_sd(kind, oracle_sd)
    rows_np, cols_np = _inputs(kind, 7)
    eng = _engine(sd, handle)
    try:
        eng.set_skip_mask(mask)
        errs = _check(eng, sd, kind, rows_np, cols_np, what=name + " / control")       # the same inputs without a plant
        print(name, "control", " ".join("%s %.3g" % kv for kv in errs.items()))
        fails = []
        for pname, a, b, square in nf.plants(rows_np, cols_np):
            got = _check_plant(eng, sd, kind, a, b, square, "%s / %s" % (name, pname))
            print("%s / %s: %s" % (name, pname, "ok" if not got else "%d failures" % len(got)))
            fails += got
        print("\n".join(fails))
        assert not fails, fails
    finally:
        eng.close()


def _nan_graph_plants(kind):
    rows_np, cols_np = _inputs(kind, 7)
    return [p for p in nf.plants(rows_np, cols_np) if p[0].startswith("NaN graphs")]


@pytest.mark.parametrize("handle", HANDLES, ids=IDS)
def test_consumers_never_report_a_nan_graph(oracle_sd, handle):
    """Whole-graph NaN plants (one row graph, one column graph) through every consumer.  Each asserts the consequence,
    counted from the plant and the labels, not agreement with the library's own matrix."""
    name, kind, mask = handle
    sd = _base_sd(kind, oracle_sd)
    eng = _engine(sd, handle)
    g = np.random.default_rng(11)
    try:
        eng.set_skip_mask(mask)
        for pname, a, b, _ in _nan_graph_plants(kind):
            what = "%s / %s" % (name, pname)
            (pr,), (pc,) = _bad_graphs(a), _bad_graphs(b)
            r, m = a.shape[0], b.shape[0]
            rows, cols = _dev(a), _dev(b)
            healthy = np.ones((r, m), dtype=bool)
            healthy[pr], healthy[:, pc] = False, False
            other = np.delete(np.arange(r), pr)
            # ---- top-k, small and large k: the NaN row reports nothing, the NaN column is never reported, and the
            #      other rows report every healthy column there is
            for fn, k in ((eng.score_topk, 1), (eng.score_topk, 16), (eng.score_topk_large, 17), (eng.score_topk_large, m)):
                v, i = fn(rows, cols, k=k)
                assert (i[pr] == -1).all() and (v[pr] == -INF).all(), (what, fn.__name__, k, "the NaN row reports")
                assert (i != pc).all(), (what, fn.__name__, k, "the NaN column is reported")
                assert not torch.isnan(v).any(), (what, fn.__name__, k)
                assert ((i[other] >= 0).sum(dim=1) == min(k, m - 1)).all(), (what, fn.__name__, k, "healthy pairs lost")
            # ---- mining: random planar poses, both classes populated in every row
            cxz = g.uniform(-15.0, 15.0, size=(m, 2))
            rxz = g.uniform(-15.0, 15.0, size=(r, 2))
            d = np.sqrt(((rxz[:, None] - cxz[None]) ** 2).sum(-1))
            for positives, empty in ((False, -INF), (True, INF)):
                v, i = eng.score_mine(rows, cols, cxz, k=16, positives=positives, row_pose=rxz)    # (self_r = r: c != r)
                assert (i[pr] == -1).all() and (v[pr] == empty).all(), (what, "score_mine", positives)
                assert (i != pc).all() and not torch.isnan(v).any(), (what, "score_mine", positives)
                n_cls = ((d <= 3.0) if positives else (d >= 20.0)) & healthy & (np.arange(m)[None] != np.arange(r)[:, None])
                assert np.array_equal((i >= 0).sum(dim=1).cpu().numpy(), np.minimum(16, n_cls.sum(axis=1))), \
                    (what, "score_mine", positives, "healthy pairs lost")
            # ---- range retrieval at -inf: exactly the pairs of two healthy graphs
            ar, ac, av, rp = eng.score_above(rows, cols, -INF)
            assert ar.numel() == (r - 1) * (m - 1) == int(rp[-1]), (what, "score_above", ar.numel())
            got = np.zeros((r, m), dtype=bool)
            got[ar.cpu().numpy(), ac.cpu().numpy()] = True
            assert np.array_equal(got, healthy) and not torch.isnan(av).any(), (what, "score_above")
            # ---- the evaluation counters: the skipped bins = the labelled pairs of a NaN graph, counted from the labels
            gt_np = g.integers(-1, 2, size=(r, m)).astype(np.int8)
            gt = torch.from_numpy(gt_np)
            pos, bad = eng.score_positives(rows, cols, gt=gt)
            assert bad == int(((gt_np == 1) & ~healthy).sum()) > 0, (what, "score_positives skipped", bad)
            assert pos.numel() == int(((gt_np == 1) & healthy).sum()) and not torch.isnan(pos).any(), (what, "positives")
            counts, skipped, _ = eng.score_threshold_counts(rows, cols, [0.25, 0.5, 0.75], gt=gt)
            assert skipped == int(((gt_np == 0) & ~healthy).sum()) > 0, (what, "score_threshold_counts skipped", skipped)
            assert int(counts.sum()) == int(((gt_np == 0) & healthy).sum()), (what, "score_threshold_counts")
            # ---- the sequence filter: Q is NaN exactly where seq_ref says so for the reference's NaN pattern
            cls, ref = nf.classes(sd, a, b)
            for L in (1, 4):
                qnan = np.isnan(seq_ref.seq_filter(ref["score"].astype(np.float32), L, 0, True, True)[0])
                assert qnan[pr].all() and qnan[:, pc].all() and (L > 1 or np.array_equal(qnan, ~healthy))
                sr, sc_, sv, sdir, srp = eng.score_seq_above(rows, cols, L, -INF)
                got = np.zeros((r, m), dtype=bool)
                got[sr.cpu().numpy(), sc_.cpu().numpy()] = True
                assert np.array_equal(got, ~qnan) and not torch.isnan(sv).any(), (what, "score_seq_above", L)
                v, i, _ = eng.score_seq_topk(rows, cols, L, k=m)
                i_np = i.cpu().numpy()
                assert np.array_equal((i_np >= 0).sum(axis=1), (~qnan).sum(axis=1)), (what, "score_seq_topk", L)
                rr = np.repeat(np.arange(r), m).reshape(r, m)
                assert not qnan[rr[i_np >= 0], i_np[i_np >= 0]].any() and not torch.isnan(v).any(), (what, "seq_topk", L)
    finally:
        eng.close()


ROW_BLOCK_M = 262144        # 64 MB / (4 M) = 64 rows a block (test_gpu_row_blocks' thin shape): 150 rows = 64 + 64 + 22


@pytest.mark.parametrize("where", [5, 70, 149], ids=["first block", "interior block", "last block"])
@pytest.mark.parametrize("handle", HANDLES[1:], ids=IDS[1:])
def test_row_blocked_epilogues(oracle_sd, handle, where):
    """The row-block fallback of the wide-range and any-shape handles in three blocks, a NaN row graph in one of them and
    a NaN column graph: the NaN row reports nothing in whichever block it lies, the rows of the other blocks lose no
    healthy pair, and what they report is the float64 score of that pair."""
    name, kind, mask = handle
    sd = _base_sd(kind, oracle_sd)
    r, m, pc = 150, ROW_BLOCK_M, 777
    f, s = (48, 1.0) if kind == "any" else (32, 4.0)
    gen = torch.Generator().manual_seed(where)
    rows, cols = torch.randn(r, f, generator=gen) * s, torch.randn(m, f, generator=gen) * s
    nf.plant_bits(rows.numpy(), (where, slice(None)), nf.QNAN_POS)
    nf.plant_bits(cols.numpy(), (pc, 0), nf.QNAN_NEG)
    rows_np, cols_np = rows.numpy().copy(), cols.numpy().copy()
    rows, cols = rows.cuda(), cols.cuda()
    eng = _engine(sd, handle)
    try:
        eng.set_skip_mask(mask)
        other = np.delete(np.arange(r), where)
        v, i = eng.score_topk(rows, cols, k=1)
        assert int(i[where, 0]) == -1 and float(v[where, 0]) == -INF
        assert (i != pc).all() and (i[other] >= 0).all() and not torch.isnan(v).any()
        i_np = i[:, 0].cpu().numpy()
        ref = score_ref.tail(sd, rows_np[other], cols_np[i_np[other]])["score"]
        d = np.abs(v[:, 0].cpu().numpy()[other].astype(np.float64) - np.diagonal(ref))
        assert (d <= BAR).all(), (name, "top-1 value vs float64", float(d.max()))
        rp = eng.score_above(rows, cols, -INF, capacity=0)[3].cpu().numpy()
        per_row = np.diff(rp)
        assert per_row[where] == 0 and (per_row[other] == m - 1).all(), (name, "score_above row counts")
    finally:
        eng.close()


def test_row_blocked_launches_of_the_tuned_handle(oracle_sd):
    """The tuned handle splits score_above / _positives / _threshold_counts into launches of 131 072 rows: three
    launches, a NaN row graph in each in turn."""
    ab_rows = 131072
    r, m = 2 * ab_rows + 37, 40
    gen = torch.Generator().manual_seed(3)
    base, cols = (torch.randn(r, 32, generator=gen) * 4.0), (torch.randn(m, 32, generator=gen) * 4.0).cuda()
    gt_np = np.random.default_rng(5).integers(-1, 2, size=(r, m)).astype(np.int8)
    gt = torch.from_numpy(gt_np).cuda()
    eng = _engine(oracle_sd, HANDLES[0])
    try:
        for where in (9, ab_rows + 1000, r - 1):
            rows = base.clone()
            nf.plant_bits(rows.numpy(), (where, slice(None)), nf.QNAN_POS)
            rows = rows.cuda()
            per_row = np.diff(eng.score_above(rows, cols, -INF, capacity=0)[3].cpu().numpy())
            assert per_row[where] == 0 and per_row.sum() == (r - 1) * m, (where, "score_above row counts")
            pos, bad = eng.score_positives(rows, cols, gt=gt)
            assert bad == int((gt_np[where] == 1).sum()) > 0 and pos.numel() == int((gt_np == 1).sum()) - bad, where
            assert not torch.isnan(pos).any()
            counts, skipped, _ = eng.score_threshold_counts(rows, cols, [0.5], gt=gt)
            assert skipped == int((gt_np[where] == 0).sum()) > 0, where
            assert int(counts.sum()) == int((gt_np == 0).sum()) - skipped, where
    finally:
        eng.close()


@pytest.fixture(scope="module")
def model(ckpt_path):
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    trainer.model.eval()
    return trainer.model


def test_model_score_all_pairs(model, oracle_sd):
    rows_np, cols_np = _inputs("f16", 7)
    fails = []
    for pname, a, b, square in nf.plants(rows_np, cols_np):
        cls, ref = nf.classes(oracle_sd, a, b)
        rows = _dev(a)
        got = model.score_all_pairs(rows, rows if square else _dev(b)).cpu().numpy()
        bad = nf.violations(got, cls, ref, np.full(cls.shape, BAR))
        if bad.any():
            fails.append((pname, int(bad.sum()), int((bad & (cls == nf.MUST_NAN)).sum())))
    assert not fails, fails


def test_place_database_never_returns_a_nan_frame(model):
    from sg_pr_amd import synth
    from sg_pr_amd.place_db import PlaceDatabase
    c, l, _ = synth.make_graphs(48, 100, 20, 90, 2, kitti_like=True)
    first = PlaceDatabase(model, capacity=64)
    first.add(c[:40], l[:40])
    vec = first.pooled.clone()
    assert torch.isfinite(vec).all()
    vec[7] = float("nan")                                   # a stored frame whose embed broke its node promise
    db = PlaceDatabase(model, capacity=64)
    db.append_pooled(vec)
    for k in (1, 16):
        v, i = db.query(c[40:], l[40:], k=k)
        assert (i != 7).all() and (i >= 0).all() and not torch.isnan(v).any(), k
    v, i = db.query(c[40:], l[40:], k=40)                   # (k beyond 16: the large-k selection)
    assert (i != 7).all() and ((i >= 0).sum(dim=1) == 39).all() and not torch.isnan(v).any()
    v, i = db.query_ids([7, 8], k=4)                        # the NaN frame as the query: nothing
    assert (i[0] == -1).all() and (i[1] != 7).all() and (i[1] >= 0).all()


@pytest.mark.parametrize("f,t", [(32, 16), (48, 20)], ids=["built shape", "any width"])
def test_standalone_ntn(oracle_sd, f, t):
    """engine.ntn (sgpr_ntn / sgpr_ntn_any): a NaN in either vector of a pair is NaN in every neuron of that pair, and
    no other pair's bits move."""
    from sg_pr_amd import engine
    if (f, t) == (32, 16):
        p = score_ref.tail_weights(oracle_sd)
        w, wb, bias = (torch.from_numpy(p[k]).float().cuda() for k in ("w", "wb", "bias"))
    else:
        gen = torch.Generator().manual_seed(f)
        w, wb, bias = ((torch.randn(*s, generator=gen) * c).cuda() for s, c in (((f, f, t), 1.0 / f), ((t, 2 * f), 0.125), ((t,), 1.0)))
    g = np.random.default_rng(f)
    e1, e2 = g.normal(0, 1.0, size=(23, f)).astype(np.float32), g.normal(0, 1.0, size=(23, f)).astype(np.float32)
    clean = engine.ntn(w, wb, bias, _dev(e1), _dev(e2))
    assert clean.shape == (23, t) and torch.isfinite(clean).all() and (clean > 0).any()
    ix = nf.element_indices(f)
    a, b = e1.copy(), e2.copy()
    nf.plant_bits(a, (3, slice(None)), nf.QNAN_POS)
    nf.plant_bits(b, (5, slice(None)), nf.QNAN_NEG)
    for pair, i, bits in zip((8, 9, 10, 22), ix, (nf.QNAN_POS, nf.QNAN_NEG, nf.QNAN_NEG, nf.QNAN_POS)):
        nf.plant_bits(a if pair % 2 else b, (pair, i), bits)
    got = engine.ntn(w, wb, bias, _dev(a), _dev(b))
    planted = np.zeros(23, dtype=bool)
    planted[[3, 5, 8, 9, 10, 22]] = True
    pt = torch.from_numpy(planted).cuda()
    assert torch.isnan(got[pt]).all(), ("a NaN pair with a finite neuron", torch.isnan(got[pt]).sum(dim=1).tolist())
    assert torch.equal(got[~pt], clean[~pt])
