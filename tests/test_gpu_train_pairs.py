"""The all-pairs training tail (sg_pr_amd.train.PairsTail / pairs_tail / train_loss_in_batch, csrc/sgpr_train_pairs.hip) on
the GPU against the float64 formulation of tests/train_pairs_ref.py, with the same formulation in fp32 torch ops on the
GPU as the yardstick of what fp32 can give; the inference engine's predictions; edge cases; determinism; today's step
and a whole in-batch step against tests/train_ref.py; the fitter's in-batch modes; activation memory.

Error rule (tests 1, 2, 4, 7): err(x) = |x - ref| / |ref| for tensors, |x - ref| / max(1, |ref|) for the loss; the op
passes when err(op) <= max(4 err(fp32 torch), 1e-6) and stays inside 1e-4 (pred) / 2e-3 (gradients)."""
import ctypes
import io
import json
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))

GRADS = ("rep",) + ("W", "V", "b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


def _args(**kw):
    from sg_pr_amd.parser_sg import sgpr_args
    a = sgpr_args()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _golden_plus_synth(n_synth, seed=0, node_num=100):
    from sg_pr_amd import synth
    from sg_pr_amd.sg_net import pack_graph
    from sg_pr_amd.utils import read_graph
    cs, ls = [], []
    for name in ("0", "250", "3"):
        d = read_graph(os.path.join(GOLDEN, "data", name + ".json"))
        c, l = pack_graph(d["centers"], d["nodes"], node_num)
        cs.append(c)
        ls.append(l)
    c, l, _ = synth.make_graphs(n_synth, node_num, 20, node_num - 10, seed, kitti_like=True)
    return np.concatenate((np.stack(cs), c)), np.concatenate((np.stack(ls), l))


def _model(sd, train=True):
    from sg_pr_amd.sg_net import SG
    m = SG(_args(), 12)
    m.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in sd.items()})
    m = m.cuda()
    return m.train() if train else m.eval()


def _release_sd(oracle):
    with zipfile.ZipFile(os.path.join(GOLDEN, "release_model.zip")) as z:
        name = sorted(n for n in z.namelist() if n.endswith("model.pth"))[0]
        return oracle.load_checkpoint(io.BytesIO(z.read(name)))


_POOLED = {}


def _pooled(key, sd, n=1024):
    """Real pooled vectors: the train-mode embedding + attention of the 3 golden graphs + synthetic ones -> [n, 32]."""
    from sg_pr_amd.train import attention, dense_features, embed_train
    if key not in _POOLED:
        centers, labels = _golden_plus_synth(n - 3)
        model = _model(sd)
        feats = dense_features(torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda())
        with torch.no_grad():
            emb, _ = embed_train(model, feats, updates=0)
            rep, _ = attention(model.attention, emb)
        _POOLED[key] = rep[:, :, 0].contiguous()
    return _POOLED[key]


def _tail_params(sd):
    import train_pairs_ref as ref
    sd = {k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}
    return {n: sd[n].detach().clone().float() for n in ref.PARAMS}


def _random_cls(g, seed):
    rng = np.random.default_rng(seed)
    if g == 1:
        return torch.tensor([[1]], dtype=torch.uint8)
    if g == 2:
        return torch.tensor([[0, 1], [2, 1]], dtype=torch.uint8)
    cls = rng.integers(0, 3, size=(g, g)).astype(np.uint8)
    cls[0, 1], cls[1, 0], cls[0, 2] = 0, 1, 2                 # all three values, asymmetric
    return torch.from_numpy(cls)


def _relerr(a, b):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _run_op(rep, cls, params, w_neg, w_pos):
    import train_pairs_ref as ref
    from sg_pr_amd.train import PairsTail
    rep = rep.detach().clone().cuda().float().requires_grad_(True)
    p = [params[n].detach().clone().cuda().requires_grad_(True) for n in ref.PARAMS]
    loss, pred, wsum = PairsTail.apply(rep, cls.cuda(), *p, w_neg, w_pos)
    assert not pred.requires_grad and not wsum.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), pred, wsum, [rep.grad] + [t.grad for t in p]


def _run_ref(rep, cls, params, w_neg, w_pos, dtype, device):
    import train_pairs_ref as ref
    rep = rep.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    p = {n: params[n].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for n in ref.PARAMS}
    loss, pred, wsum = ref.ref_pairs_loss(rep, cls, p, w_neg, w_pos, chunk=128, backward=True)
    grads = [rep.grad] + [p[n].grad for n in ref.PARAMS]
    grads = [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, [rep] + [p[n] for n in ref.PARAMS])]
    return loss, pred, wsum, grads


def _check(tag, op, y32, r64, report=None):
    """op / y32 / r64: (loss, pred, wsum, grads) of the HIP op, fp32 torch on the GPU and float64 on the CPU."""
    lines = []

    def gate(name, e_op, e_y, outer):
        lines.append("%s %-6s op %.3e  fp32-torch %.3e" % (tag, name, e_op, e_y))
        return e_op <= max(4.0 * e_y, 1e-6) and e_op <= outer

    ok = []
    den = max(1.0, abs(float(r64[0])))
    ok.append(("loss", gate("loss", abs(float(op[0]) - float(r64[0])) / den, abs(float(y32[0]) - float(r64[0])) / den,
                            float("inf"))))
    ok.append(("pred", gate("pred", _relerr(op[1], r64[1]), _relerr(y32[1], r64[1]), 1e-4)))
    ok.append(("wsum", abs(float(op[2]) - float(r64[2])) <= 1e-6 * max(1.0, float(r64[2]))))
    for name, a, y, r in zip(GRADS, op[3], y32[3], r64[3]):
        assert a.shape == r.shape, (name, a.shape, r.shape)
        assert torch.isfinite(a).all(), name
        if float(r.norm()) == 0.0:
            ok.append((name, float(a.abs().max()) <= 1e-6))
            continue
        ok.append((name, gate("d_" + name, _relerr(a, r), _relerr(y, r), 2e-3)))
    print("\n".join(lines))
    if report is not None:
        report.extend(lines)
    bad = [n for n, v in ok if not v]
    assert not bad, (tag, bad, lines)


def _three_way(tag, rep, cls, params, w_neg=1.0, w_pos=1.0):
    op = _run_op(rep, cls, params, w_neg, w_pos)
    y32 = _run_ref(rep, cls, params, w_neg, w_pos, torch.float32, "cuda")
    r64 = _run_ref(rep, cls, params, w_neg, w_pos, torch.float64, "cpu")
    _check(tag, op, y32, r64)
    return op, r64


# ------------------------------------------------------------------------------------------------ 1. op vs float64
@pytest.mark.parametrize("g", [1, 2, 37, 256, 257, 1024])
@pytest.mark.parametrize("which", ["golden", "release"])
def test_op_against_float64(g, which, oracle, oracle_sd):
    sd = oracle_sd if which == "golden" else _release_sd(oracle)
    rep = _pooled(which, sd)[:g]
    _three_way("%s G=%d" % (which, g), rep, _random_cls(g, g), _tail_params(sd), w_neg=1.0, w_pos=2.5)


# ------------------------------------------------------------------------------------------------ 2. other widths
@pytest.mark.parametrize("f,t,h", [(64, 32, 32), (20, 5, 7), (128, 64, 64)])
def test_other_widths(f, t, h):
    import train_pairs_ref as ref
    gen = torch.Generator().manual_seed(f * 1000 + t)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen) * scale

    g = 50
    params = dict(zip(ref.PARAMS, (rn(f, f, t, scale=1.0 / f), rn(t, 2 * f, scale=(2 * f) ** -0.5), rn(t, 1, scale=0.1),
                                   rn(h, t, scale=t ** -0.5), rn(h, scale=0.1), rn(1, h, scale=h ** -0.5),
                                   rn(1, scale=0.1))))
    _three_way("F=%d T=%d H=%d" % (f, t, h), rn(g, f), _random_cls(g, f), params, w_neg=0.7, w_pos=1.3)


# ------------------------------------------------------------------------------------------------ 3. inference engine
def test_predictions_are_the_inference_engines(oracle_sd):
    from sg_pr_amd.train import pairs_tail
    rep = _pooled("golden", oracle_sd)[:256]
    model = _model(oracle_sd, train=False)
    with torch.no_grad():
        want = model.score_all_pairs(rep, rep)
    cls = torch.full((256, 256), 2, dtype=torch.uint8)
    _, pred, _ = pairs_tail(rep, cls, model.tensor_network, model.fully_connected_first, model.scoring_layer)
    torch.cuda.synchronize()
    err = float((pred - want).abs().max())
    print("pred vs Engine.score_all_pairs: max |d| %.3e" % err)
    assert err <= 1e-4


# ------------------------------------------------------------------------------------------------ 4. edge cases
def test_edge_cases(oracle_sd):
    g = 37
    rep = _pooled("golden", oracle_sd)[:g]
    params = _tail_params(oracle_sd)
    none = torch.full((g, g), 2, dtype=torch.uint8)
    # no labelled pair (also with values beyond 2): loss 0, zero gradients, everything finite
    for cls in (none, torch.full((g, g), 255, dtype=torch.uint8)):
        loss, pred, wsum, grads = _run_op(rep, cls, params, 1.0, 1.0)
        assert float(loss) == 0.0 and float(wsum) == 0.0 and torch.isfinite(pred).all()
        assert all(float(x.abs().max()) == 0.0 for x in grads)
    only_neg, only_pos, one = none.clone(), none.clone(), none.clone()
    only_neg[_random_cls(g, 1) == 0] = 0
    only_pos[_random_cls(g, 2) == 1] = 1
    one[5, 9] = 1
    _three_way("only negatives", rep, only_neg, params)
    _three_way("only positives", rep, only_pos, params)
    (loss, pred, wsum, _), _ = _three_way("one labelled pair", rep, one, params)
    assert float(wsum) == 1.0
    assert abs(float(loss) + float(torch.log(pred[5, 9]))) <= 1e-6 * max(1.0, float(loss))
    (_, _, wsum, _), _ = _three_way("w_pos = 0", rep, _random_cls(g, 3), params, w_neg=1.0, w_pos=0.0)
    assert float(wsum) == float((_random_cls(g, 3) == 0).sum())
    loss, _, wsum, grads = _run_op(rep, only_pos, params, 1.0, 0.0)           # every weight 0
    assert float(loss) == 0.0 and float(wsum) == 0.0 and all(float(x.abs().max()) == 0.0 for x in grads)
    zero_row = rep.clone()
    zero_row[4] = 0.0
    _three_way("a zero row", zero_row, _random_cls(g, 4), params)
    # a saturated head (scoring_layer scaled to weight 0, bias +60 / -200): s rounds to 1 / 0 in fp32 for every pair; the
    # loss is the clamp's 100 per wrong pair, the gradient exactly 0
    cls = _random_cls(g, 5)
    n_neg, n_pos = int((cls == 0).sum()), int((cls == 1).sum())
    for bias, value, wrong in ((60.0, 1.0, n_neg * 1.0), (-200.0, 0.0, n_pos * 2.0)):
        sat = dict(params)
        sat["scoring_layer.weight"] = params["scoring_layer.weight"] * 0.0
        sat["scoring_layer.bias"] = torch.tensor([bias])
        loss, pred, wsum, grads = _run_op(rep, cls, sat, 1.0, 2.0)
        assert (pred == value).all()
        want = 100.0 * wrong / (n_neg + 2.0 * n_pos)
        y32 = _run_ref(rep, cls, sat, 1.0, 2.0, torch.float32, "cuda")
        print("saturated at %g: loss %.6f, expected %.6f, fp32 torch %.6f" % (value, float(loss), want, float(y32[0])))
        assert abs(float(loss) - want) <= 1e-6 * want and abs(float(y32[0]) - want) <= 1e-5 * want
        assert all(float(x.abs().max()) == 0.0 for x in grads)
        assert all(float(x.abs().max()) == 0.0 for x in y32[3])


# ------------------------------------------------------------------------------------------------ 5. determinism
def _raw(lib, rep, cls, p, w_neg, w_pos, ws_fill, stream):
    """The C entry points directly, on `stream`, with a caller-made workspace filled with ws_fill -> every output."""
    from sg_pr_amd import engine
    g, f = rep.shape
    t, h = p[0].shape[2], p[3].shape[0]
    ptr = engine._ptr
    with torch.cuda.stream(stream):
        ws_bytes = int(lib.sgpr_pairs_train_workspace_bytes(g, f, t, h))
        ws = torch.full((ws_bytes,), ws_fill, dtype=torch.uint8, device="cuda")
        pred = torch.full((g, g), float("nan"), device="cuda")
        loss = torch.full((1,), float("nan"), device="cuda")
        wsum = torch.full((1,), float("nan"), device="cuda")
        st = ctypes.c_void_p(stream.cuda_stream)
        rc = lib.sgpr_pairs_train_forward(ptr(rep), *[ptr(x) for x in p], ptr(cls), w_neg, w_pos, g, f, t, h, ptr(pred),
                                          ptr(loss), ptr(wsum), ptr(ws), ws_bytes, st)
        assert rc == 0, lib.sgpr_last_error()
        ws.fill_(255 - ws_fill)
        dloss = torch.ones(1, device="cuda")
        grads = [torch.full_like(x, float("nan")) for x in [rep] + list(p)]
        rc = lib.sgpr_pairs_train_backward(ptr(dloss), ptr(wsum), ptr(pred), ptr(rep), *[ptr(x) for x in p], ptr(cls),
                                           w_neg, w_pos, g, f, t, h, *[ptr(x) for x in grads], ptr(ws), ws_bytes, st)
        assert rc == 0, lib.sgpr_last_error()
    stream.synchronize()
    return [loss, wsum, pred] + grads


def test_determinism_and_statelessness(oracle_sd):
    import train_pairs_ref as ref
    from sg_pr_amd import engine
    lib = engine.load_library()
    params = _tail_params(oracle_sd)
    p = [params[n].cuda().contiguous() for n in ref.PARAMS]
    for g in (37, 257):
        rep = _pooled("golden", oracle_sd)[:g].contiguous()
        cls = _random_cls(g, 7).cuda()
        torch.cuda.synchronize()
        a = _raw(lib, rep, cls, p, 1.0, 2.5, 0, torch.cuda.current_stream())
        b = _raw(lib, rep, cls, p, 1.0, 2.5, 255, torch.cuda.Stream())
        for x, y in zip(a, b):
            assert torch.isfinite(x).all()
            assert torch.equal(x, y)
        # and the autograd binding gives the same bits as the raw calls
        op = _run_op(rep, cls, params, 1.0, 2.5)
        assert torch.equal(op[0].reshape(1), a[0]) and torch.equal(op[1], a[2])
        for x, y in zip(op[3], a[3:]):
            assert torch.equal(x.reshape(-1), y.reshape(-1))


# ------------------------------------------------------------------------------------------------ 6. today's step
def _buffers_match(model, before, stats_list):
    import train_ref
    want = train_ref.running_after({k: v for k, v in before.items() if "running" in k or "num_batches" in k}, stats_list)
    got = model.state_dict()
    for k, v in want.items():
        if "num_batches" in k:
            assert int(got[k]) == int(v), k
        else:
            assert _relerr(got[k], v) <= 1e-5, (k, _relerr(got[k], v))


def _grads_match(model, p):
    for name, prm in model.named_parameters():
        ref = p[name].grad
        assert prm.grad is not None and ref is not None, name
        if float(ref.norm()) == 0.0:
            assert float(prm.grad.abs().max()) <= 1e-6, name
            continue
        assert _relerr(prm.grad, ref) <= 2e-3, (name, _relerr(prm.grad, ref))


def _todays_step_in_the_op(sd):
    from sg_pr_amd.train import dense_features, train_loss_in_batch
    import train_ref
    centers, labels = _golden_plus_synth(13)
    feats = dense_features(torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda())
    target = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0], device="cuda")
    cls = torch.full((16, 16), 2, dtype=torch.uint8)
    for q in range(8):
        cls[q, q + 8] = cls[q + 8, q] = int(target[q])
    model = _model(sd)
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    loss, pred, lists = train_loss_in_batch(model, feats, cls.cuda(), 1.0, 1.0)
    loss.backward()
    p = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point()) for k, v in before.items()}
    loss_r, pred_r, stats = train_ref.train_step_loss(p, feats.cpu().double(), target.cpu().double(),
                                                      [i.cpu() for i in lists])
    loss_r.backward()
    q = torch.arange(8)
    listed = torch.cat((pred[q, q + 8], pred[q + 8, q]))
    print("today's step in the op: loss %.8f ref %.8f, pred err %.3e" % (loss.item(), loss_r.item(),
                                                                           _relerr(listed, pred_r)))
    assert abs(loss.item() - loss_r.item()) <= 1e-5, (loss.item(), loss_r.item())
    assert _relerr(listed, pred_r) <= 1e-4
    _grads_match(model, p)
    _buffers_match(model, before, stats)


def test_todays_step_from_golden_model(oracle_sd):
    _todays_step_in_the_op(oracle_sd)


def test_todays_step_from_release_checkpoint(oracle):
    _todays_step_in_the_op(_release_sd(oracle))


# ------------------------------------------------------------------------------------------------ 7. in-batch step
WORLD_IDS = np.concatenate((np.arange(0, 90, 6), [1]))       # 16 scans of the world: 10 / 86 ... all three classes


def _world():
    from sg_pr_amd import synth
    c, l, _, poses = synth.world_sequence(num_graphs=90, node_num=100, seed=5)
    return c, l, poses


def _ref_in_batch(p, feats, cls, lists, w_neg, w_pos):
    """train_ref.conv_pass + attention + the pairs reference in p's dtype, on feats' device -> (loss, pred, stats)."""
    import train_pairs_ref as ref
    import train_ref
    emb, stats = train_ref.conv_pass(p, feats, lists)
    ctx = torch.tanh(torch.mean(torch.matmul(emb, p["attention.weight_matrix"]), dim=1))
    s = torch.sigmoid(torch.matmul(emb, ctx.unsqueeze(-1)))
    rep = torch.matmul(emb.permute(0, 2, 1), s)[:, :, 0]
    loss, pred, _ = ref.ref_pairs_loss(rep, cls, p, w_neg, w_pos, chunk=1 << 20)
    return loss, pred, stats


@pytest.mark.parametrize("mode", ["all", "balanced"])
def test_whole_in_batch_step_against_float64(mode, oracle_sd):
    from sg_pr_amd.train import dense_features, pair_classes, train_loss_in_batch
    c, l, poses = _world()
    cls_np = pair_classes(poses[:, [3, 11]], WORLD_IDS)
    n_pos, n_neg = int((cls_np == 1).sum()), int((cls_np == 0).sum())
    assert n_pos > 0 and n_neg > 0 and int((cls_np == 2).sum()) > 16
    w_pos = n_neg / n_pos if mode == "balanced" else 1.0
    cls = torch.from_numpy(cls_np)
    feats = dense_features(torch.from_numpy(c[WORLD_IDS]).cuda(), torch.from_numpy(l[WORLD_IDS]).cuda())
    model = _model(oracle_sd)
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    loss, pred, lists = train_loss_in_batch(model, feats, cls.cuda(), 1.0, w_pos)
    loss.backward()
    p = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point()) for k, v in before.items()}
    loss_r, pred_r, stats = _ref_in_batch(p, feats.cpu().double(), cls, [i.cpu() for i in lists], 1.0, w_pos)
    loss_r.backward()
    with torch.no_grad():
        p32 = {k: v.detach().cuda() for k, v in before.items()}
        loss_y, _, _ = _ref_in_batch(p32, feats, cls, lists, 1.0, w_pos)
    loss_r = loss_r.detach()
    den = max(1.0, abs(float(loss_r)))
    e_op, e_y = abs(float(loss) - float(loss_r)) / den, abs(float(loss_y) - float(loss_r)) / den
    print("in-batch step (%s, %d positives, %d negatives): loss %.8f ref %.8f  err op %.3e fp32-torch %.3e  pred %.3e"
          % (mode, n_pos, n_neg, float(loss), float(loss_r), e_op, e_y, _relerr(pred, pred_r)))
    assert e_op <= max(4.0 * e_y, 1e-6), (e_op, e_y)
    assert _relerr(pred, pred_r) <= 1e-4
    _grads_match(model, p)
    _buffers_match(model, before, [stats, stats])


# ------------------------------------------------------------------------------------------------ 8. fitter
def _pairs_of_world(num_graphs=90, seed=5, p_thresh=3.0):
    c, l, poses = _world()
    xz = poses[:, [3, 11]]
    d = np.sqrt(((xz[:, None] - xz[None]) ** 2).sum(-1))
    i, j = np.triu_indices(num_graphs, 1)
    pos = np.nonzero(d[i, j] <= p_thresh)[0]
    neg = np.nonzero(d[i, j] >= 20.0)[0]
    rng = np.random.default_rng(seed)
    return c, l, poses, i, j, pos, rng.choice(neg, size=min(len(neg), len(pos)), replace=False)


def _fitter(tmp_path, seed=0, n_train=48, batch=16, augment=True, fitter_kw=None, **kw):
    from sg_pr_amd.train import PairSet, SGFitter
    c, l, poses, i, j, pos, neg = _pairs_of_world()
    pick = np.concatenate((pos[:n_train // 2], neg[:n_train // 2]))
    pairs = np.stack((i[pick], j[pick]), axis=1)
    data = PairSet(c, l, poses, pairs, pairs[::3])
    f = SGFitter(_args(batch_size=batch, logdir=str(tmp_path), epochs=1, **kw), seed=seed, data=data, **(fitter_kw or {}))
    f.augment = augment
    return f


def _five_steps(f):
    from sg_pr_amd.train import batches_of
    for ids in (batches_of(len(f.data.train_pairs), 16, f.rng) * 2)[:5]:
        f.step(ids)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in f.model.state_dict().items()}


def test_in_batch_off_is_the_default_fitter(tmp_path):
    a = _five_steps(_fitter(tmp_path, seed=11))
    b = _five_steps(_fitter(tmp_path, seed=11, fitter_kw={"in_batch": "off"}))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        _fitter(tmp_path, fitter_kw={"in_batch": "some"})


@pytest.mark.parametrize("mode", ["all", "balanced"])
def test_in_batch_same_seed_same_state(tmp_path, mode):
    sds = [_five_steps(_fitter(tmp_path, seed=11, fitter_kw={"in_batch": mode})) for _ in range(2)]
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k
    off = _five_steps(_fitter(tmp_path, seed=11))
    assert any(not torch.equal(off[k], sds[0][k]) for k in off)


def test_log_carries_the_pair_counts(tmp_path):
    from sg_pr_amd.train import batches_of, pair_classes
    f = _fitter(tmp_path, seed=2, fitter_kw={"in_batch": "balanced"})
    order = batches_of(len(f.data.train_pairs), 16, np.random.default_rng(2))
    f.fit(epochs=1)
    recs = [json.loads(line) for line in open(os.path.join(str(tmp_path), "train_log.jsonl"))]
    steps = [r for r in recs if "pairs_in_loss" in r]
    assert len(steps) == len(order) == 3
    for r, ids in zip(steps, order):
        pairs = f.data.train_pairs[ids]
        cls = pair_classes(f.data.xz, np.concatenate((pairs[:, 0], pairs[:, 1])), None, f.data.p_thresh)
        assert r["pairs_in_loss"] == int((cls <= 1).sum()) > 2 * len(ids)
        assert r["positives"] == int((cls == 1).sum()) and r["negatives"] == int((cls == 0).sum())
        assert np.isfinite(r["loss"])
    off = _fitter(tmp_path / "off", seed=2)
    off.fit(epochs=1)
    assert "pairs_in_loss" not in open(os.path.join(str(tmp_path / "off"), "train_log.jsonl")).read()


def test_in_batch_overfit_decreases(tmp_path):
    f = _fitter(tmp_path, seed=3, n_train=32, batch=32, augment=False, learning_rate=1e-4, fitter_kw={"in_batch": "all"})
    ids = np.arange(len(f.data.train_pairs))
    losses = [f.step(ids) for _ in range(60)]
    print("in-batch overfit losses", losses[0], losses[-1], f.last_step)
    assert f.last_step["pairs_in_loss"] > 64
    assert losses[-1] < losses[0], (losses[0], losses[-1])


def test_in_batch_checkpoint_loads_into_inference_and_oracle(tmp_path, oracle):
    from sg_pr_amd import sg_net
    f = _fitter(tmp_path, seed=1, fitter_kw={"in_batch": "all"})
    f.fit(epochs=1)
    path = os.path.join(str(tmp_path), "0.pth")
    assert os.path.exists(path)
    sd_raw = torch.load(path, map_location="cpu")
    assert len(sd_raw) == 50 and all(k.startswith("module.") for k in sd_raw)
    args = _args(model=path)
    trainer = sg_net.SGTrainer(args, False)
    pairs = [[os.path.join(GOLDEN, "data", a + ".json"), os.path.join(GOLDEN, "data", b + ".json")]
             for a, b in (("0", "250"), ("0", "3"), ("250", "250"))]
    pred, gt = trainer.eval_batch_pair(pairs)
    sd = oracle.load_checkpoint(path)
    ref, gt_ref = oracle.eval_batch_pair(sd, pairs, args.node_num, args.K, args.p_thresh)
    assert float(np.max(np.abs(pred - ref))) <= 1e-4
    assert np.array_equal(gt, gt_ref)


# ------------------------------------------------------------------------------------------------ 9. memory
def test_activation_memory_vs_torch_ops_tail(oracle_sd):
    import train_pairs_ref as ref
    from sg_pr_amd.train import pairs_tail
    g = 256
    model = _model(oracle_sd)
    rep0 = _pooled("golden", oracle_sd)[:g].clone()
    cls = _random_cls(g, 9).cuda()

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def hip():
        rep = rep0.clone().requires_grad_(True)
        loss, _, _ = pairs_tail(rep, cls, model.tensor_network, model.fully_connected_first, model.scoring_layer)
        loss.backward()

    def torch_ops():
        rep = rep0.clone().requires_grad_(True)
        loss, _, _ = ref.gathered_pairs_loss(rep, cls, model)
        loss.backward()

    hip()
    model.zero_grad(set_to_none=True)
    m_hip = peak(hip)
    model.zero_grad(set_to_none=True)
    m_torch = peak(torch_ops)
    print("tail activation memory at G = 256: HIP %.2f MB, torch ops %.1f MB, ratio %.1f"
          % (m_hip / 2 ** 20, m_torch / 2 ** 20, m_torch / max(m_hip, 1)))
    assert m_hip * 3 <= m_torch
