"""Every scoring entry point at the edges of the f16 range, against the float64 reference of tests/score_ref.py.

The matrix-core tails cut their operands - the head's fold fc2_w[o] fc1_w[o][t] among them - into f16 planes.  Checkpoint
variants move the fold to both edges of that range: a power-of-two reparametrisation that keeps the function (c = 1/8, 8;
the fold shrinks to 1/8 of the shipped 0.13 at c = 8), a dead neuron with a fold of 1e5 (contributes exactly 0) and a
live pair of neurons whose folds of +-1e5 cancel.  Each runs on every kind of handle (tuned f16, tuned with debug bit 13,
wide-range by checkpoint, any-shape with and without debug bit 23) through score_pairs, score_pair_list, score_all_pairs,
score_all_pairs_multi, score_topk and SequenceSet, which must be finite, within the float64 bar and keep their bitwise
contracts with each other.  A second test puts the inputs at 0.97x / 1.03x of each range gate of the launch."""
import numpy as np
import pytest
import torch

import score_ref
from test_gpu_topk import _reference as _topk_reference

pytestmark = pytest.mark.gpu

BAR = 3e-6            # f16 planes and exact fp32 against float64 at input scale 1 (test_all_pairs_f16_range_guard)
BAR_BF16 = 1e-6       # the three-bf16-plane instance
EPS_COND = 2.0 ** -21  # where the head's terms are large (cancellation, the gates' edges): |dscore| <= p'(z) EPS_COND zmag
N_PAIRS = 3000


def _any_shape(sd=None):
    from sg_pr_amd import engine, sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.filters_1, args.filters_2, args.filters_3, args.tensor_neurons, args.bottle_neck_neurons = 64, 64, 48, 16, 16
    args.node_num, args.K = 64, 10
    if sd is None:
        torch.manual_seed(5)
        return {k: v.detach().clone() for k, v in sg_net.SG(args, 12).eval().state_dict().items()}
    return engine.Engine(sd, dims=engine.dims_from_args(args, 12), device=0)


def _wide_checkpoint(sd):
    """test_weights_outside_the_f16_range_take_the_wide_range_instance's construction: one live channel of
    dgcnn_s_conv2 with folded weights of 2e5."""
    sd = {k: v.clone() for k, v in sd.items()}
    key = [k for k in sd if k.endswith("dgcnn_s_conv2.0.weight")][0]
    pre = key[: -len("0.weight")]
    fold = sd[pre + "1.weight"] / torch.sqrt(sd[pre + "1.running_var"] + 1e-5)
    mag = fold.abs() * sd[key].flatten(1).abs().amax(1)
    ch = int(mag.argmax())
    sd[key][ch] *= 2e5 / float(mag[ch])
    return sd


# (name, kind, debug mask): kind f16 = the tuned handle's two-plane tail, bf16 = its three-plane instance, any = any-shape
HANDLES = [("tuned", "f16", 0), ("tuned, bit 13", "bf16", 1 << 13), ("wide checkpoint", "bf16", 0),
           ("any-shape", "any", 0), ("any-shape, bit 23", "any", 1 << 23)]


def _engine(sd, handle):
    from sg_pr_amd import engine
    name, kind, _ = handle
    if kind == "any":
        return _any_shape(sd)
    e = engine.Engine(_wide_checkpoint(sd) if name == "wide checkpoint" else sd, device=0)
    assert e.uses_f16_planes() == (name != "wide checkpoint")
    return e


def _inputs(kind, seed, r=37, m=131):
    g = np.random.default_rng(seed)
    f, s = (48, 1.0) if kind == "any" else (32, 4.0)
    return g.normal(0, s, size=(r, f)).astype(np.float32), g.normal(0, s, size=(m, f)).astype(np.float32)


def _tolerance(ref, bar, cond):
    tol = np.full(ref["score"].shape, bar)
    if cond:
        tol = tol + EPS_COND * ref["score"] * (1.0 - ref["score"]) * ref["zmag"]
    return tol


def _check(eng, sd, kind, rows_np, cols_np, cond=False, what=""):
    """Every entry point on rows x cols -> max |d| against float64 per entry point; asserts the bar and the contracts.
    cond: add the conditioning term to the bar (large head terms)."""
    r, m = rows_np.shape[0], cols_np.shape[0]
    ref = score_ref.tail(sd, rows_np, cols_np)
    head_wide = np.abs(score_ref.fold(sd)).max() >= score_ref.F16_SAFE
    tuned_f16 = kind == "f16" and not head_wide            # the tuned tail on its f16 planes
    bar_m = BAR_BF16 if (kind == "bf16" or (kind == "f16" and head_wide)) and not cond else BAR
    tol, tol_m = _tolerance(ref, BAR, cond), _tolerance(ref, bar_m, cond)
    rows, cols = torch.from_numpy(rows_np).cuda(), torch.from_numpy(cols_np).cuda()
    errs = {}

    def within(name, got, want_ref, tl):
        g_ = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(g_).all(), (what, name, "not finite")
        d = np.abs(g_ - want_ref)
        errs[name] = float(d.max())
        assert (d <= tl).all(), (what, name, float(d.max()), float((d - tl).max()))

    ii, jj = torch.meshgrid(torch.arange(r, dtype=torch.int32), torch.arange(m, dtype=torch.int32), indexing="ij")
    sp = eng.score_pairs(rows, cols, ii.reshape(-1), jj.reshape(-1)).view(r, m)
    within("score_pairs", sp, ref["score"], tol)
    mat = eng.score_all_pairs(rows, cols)
    within("score_all_pairs", mat, ref["score"], tol_m)
    # a pair list: every row count, repeated pairs
    g = np.random.default_rng(r * 1000 + m)
    i1, i2 = g.integers(0, r, N_PAIRS), g.integers(0, m, N_PAIRS)
    i1[:3], i2[:3] = 0, m - 1
    plan = eng.pair_plan(i1, i2, r, m)
    pl = eng.score_pair_list(rows, cols, plan)
    within("score_pair_list", pl, ref["score"][i1, i2], tol[i1, i2])
    t1, t2 = torch.from_numpy(i1).cuda(), torch.from_numpy(i2).cuda()
    if tuned_f16:
        assert torch.equal(pl, mat[t1, t2]), (what, "pair list != matrix entries")
    elif kind == "any":
        assert torch.equal(pl, sp[t1, t2]), (what, "pair list != score_pairs")
    else:                   # wide-range tails: the list kernel's exact fp32 arithmetic - score_pairs' to rounding
        assert (pl - sp[t1, t2]).abs().max().item() <= 1e-6 + (0 if not cond else 1e-3), what
    # more than 8 ragged jobs (two calls of the C entry point), an empty one, a padded output
    jobs = [(rows[:17], cols), (rows[:1], cols[:65]), (rows, cols[:1]), (rows[5:], cols[3:]), (rows[:0], cols),
            (rows[2:19], cols[:131]), (rows, cols, torch.empty(r, m + 7, device="cuda")[:, :m])]
    jobs = jobs + jobs[:4]
    got = eng.score_all_pairs_multi(jobs)
    for (jr, jc, *_), g_ in zip(jobs, got):
        if g_.numel():
            assert torch.equal(g_, eng.score_all_pairs(jr.contiguous(), jc.contiguous())), (what, "multi != single")
    # top-k: the matrix + top-k rows, value and index
    for k in (1, 16):
        for causal in (False, True):
            v, ix = eng.score_topk(rows, cols, k=k, window=2, causal=causal)
            wv, wi = _topk_reference(mat, k, window=2, causal=causal)
            bad = ((v != wv) & ~(torch.isinf(v) & torch.isinf(wv))) | (ix != wi)
            assert not bad.any(), (what, "topk", k, causal, [(int(a), int(b), float(v[a, b]), float(wv[a, b]), int(ix[a, b]),
                                                            int(wi[a, b])) for a, b in bad.nonzero().tolist()[:8]])
    return errs


def _sequence_sets(eng, kind):
    """SequenceSet with batch_tails=True (score_all_pairs_multi) == batch_tails=False (per sequence) on this handle."""
    from sg_pr_amd import allpairs, synth
    node_num = 64 if kind == "any" else 100
    seqs = []
    for seed, m in ((1, 40), (2, 17), (3, 70)):
        c, l, _, _ = synth.kitti_like_sequence(m, node_num, seed)
        seqs.append((torch.from_numpy(c).cuda(), torch.from_numpy(l).cuda()))
    scorer = allpairs.AllPairsScorer(embed_fn=lambda c, l: eng.embed(c, l, 10)[0], score_fn=eng.score_all_pairs)
    scorer._engine = eng
    a = allpairs.SequenceSet(scorer, seqs, batch_tails=True).run()
    b = allpairs.SequenceSet(scorer, seqs, batch_tails=False).run()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "SequenceSet batch_tails"


def _variants(sd, kind):
    rows, cols = _inputs(kind, 7)
    inputs = [(rows, cols), _inputs(kind, 8, 17, 65)]
    out = [("base", sd, False)]
    out += [("c=%g" % c, score_ref.reparametrised(sd, c), False) for c in (0.125, 8.0)]
    out.append(("dead neuron, fold 1e5", score_ref.dead_neuron_with_huge_fold(sd, inputs)[0], False))
    out.append(("cancelling folds +-1e5", score_ref.live_cancellation(sd, inputs)[0], True))
    return out, inputs


@pytest.mark.parametrize("handle", HANDLES, ids=[h[0] for h in HANDLES])
def test_every_entry_point_on_head_variants(oracle_sd, handle):
    name, kind, mask = handle
    base_sd = _any_shape() if kind == "any" else oracle_sd
    variants, inputs = _variants(base_sd, kind)
    base_pairs = {}
    for vname, sd, cond in variants:
        for rows_np, cols_np in inputs:
            ref = score_ref.tail(sd, rows_np, cols_np)
            sc = ref["score"]
            assert ((sc > 0.02) & (sc < 0.98)).mean() > 0.02, (vname, "saturated: the comparison would be vacuous")
            if vname.startswith("c="):     # the reparametrisation stays on the f16 path at these inputs
                assert score_ref.bound(ref, score_ref.ANY_SHAPE_K if kind == "any" else score_ref.TUNED_K) < 6e4
        eng = _engine(sd, handle)
        try:
            eng.set_skip_mask(mask)
            for n, (rows_np, cols_np) in enumerate(inputs):
                what = "%s / %s / %dx%d" % (name, vname, rows_np.shape[0], cols_np.shape[0])
                errs = _check(eng, sd, kind, rows_np, cols_np, cond=cond, what=what)
                print(what, " ".join("%s %.3g" % kv for kv in errs.items()))
                # the reparametrised checkpoints are the same function: the exact fp32 path gives the same bits
                rows, cols = torch.from_numpy(rows_np).cuda(), torch.from_numpy(cols_np).cuda()
                sp = eng.score_pairs(rows.repeat_interleave(cols.shape[0], 0), cols.repeat(rows.shape[0], 1))
                if vname == "base":
                    base_pairs[n] = sp
                elif vname.startswith("c="):
                    assert torch.equal(sp, base_pairs[n]), (what, "score_pairs bits")
            if vname in ("base", "dead neuron, fold 1e5"):
                _sequence_sets(eng, kind)
        finally:
            eng.close()


GATES = [("am", score_ref.F16_SAFE), ("em", score_ref.F16_SAFE), ("bound", score_ref.F16_SAFE), ("mode2", score_ref.MODE2_BOUND)]


@pytest.mark.parametrize("kind", ["f16", "any"])
def test_inputs_straddling_the_range_gates(oracle_sd, kind):
    """Inputs scaled so that each range quantity of the launch sits at 0.97x and 1.03x of its threshold (score_ref.gates:
    am, em and the bound um + K am em against 60000, um + l1 em against 1024 - the tuned tail's mode boundary), on ragged
    shapes.  The checkpoint is the c = 8 reparametrisation: four times the shipped bound on H at the same inputs, so that
    the 60000 edge of the bound is reached where 9 % of the scores are not saturated (at c = 1/8 the bound would only be
    reached at 2.8x larger inputs, where the head saturates).  am and em alone reach 60000 only at inputs ~1000x real
    ones, beyond the bound: both sides take the exact path there, and every score saturates."""
    base = _any_shape() if kind == "any" else oracle_sd
    sd = score_ref.reparametrised(base, 8.0)
    kb = score_ref.ANY_SHAPE_K if kind == "any" else score_ref.TUNED_K
    eng = _engine(sd, ("any-shape" if kind == "any" else "tuned", kind, 0))
    try:
        for quantity, thr in GATES:
            if kind == "any" and quantity == "mode2":
                continue                                   # (the any-shape tail has one form)
            for r, m in ((17, 131), (1, 65), (17, 1)):
                rows_np, cols_np = _inputs(kind, 11, r, m)
                for f in (0.97, 1.03):
                    s = score_ref.scale_to(sd, rows_np, cols_np, quantity, f * thr, kb)
                    rs, cs = rows_np * np.float32(s), cols_np * np.float32(s)
                    ref = score_ref.tail(sd, rs, cs)
                    q = dict(am=ref["am"], em=ref["em"], bound=score_ref.bound(ref, kb),
                             mode2=ref["um"] + ref["l1"] * ref["em"])[quantity]
                    assert abs(q / (f * thr) - 1.0) < 1e-3
                    if quantity in ("bound", "mode2") and r * m > 1000:
                        sc = ref["score"]
                        assert ((sc > 0.02) & (sc < 0.98)).mean() > 0.02, (quantity, f, "saturated")
                    what = "%s gate %s at %.2fx, %dx%d (scale %.4g)" % (kind, quantity, f, r, m, s)
                    errs = _check(eng, sd, kind, rs, cs, cond=True, what=what)
                    print(what, " ".join("%s %.3g" % kv for kv in errs.items()))
    finally:
        eng.close()
