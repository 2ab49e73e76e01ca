"""The all-pairs training tail off the GPU: exported symbols, host-side argument checks (no device is touched), the
workspace bound, pair_classes, the shared x-flip of augment and the float64 reference the GPU tests use.  CPU only."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

SYMS = ("sgpr_pairs_train_workspace_bytes", "sgpr_pairs_train_forward", "sgpr_pairs_train_backward")


def test_exported_symbols():
    from sg_pr_amd import engine
    lib = engine.load_library()
    for sym in SYMS:
        assert sym in engine.ABI_SYMBOLS
        getattr(lib, sym)
    with open(os.path.join(REPO, "include", "sgpr.h")) as f:
        h = f.read()
    assert "#define SGPR_TRAIN_PAIRS_MAX_GRAPHS 1024" in h
    assert lib.sgpr_abi_version() == 11


def test_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call here fails its host-side checks
    G, F, T, H = 37, 32, 16, 16
    need = lib.sgpr_pairs_train_workspace_bytes(G, F, T, H)
    assert need > 0

    def fwd(ptrs=None, g=G, f=F, t=T, h=H, wn=1.0, wp=1.0, ws=p, wb=need):
        a = [p] * 9 if ptrs is None else ptrs[:9]
        o = [p] * 3 if ptrs is None else ptrs[9:]
        return lib.sgpr_pairs_train_forward(*a, wn, wp, g, f, t, h, *o, ws, wb, None)

    def bwd(ptrs=None, g=G, f=F, t=T, h=H, wn=1.0, wp=1.0, ws=p, wb=need):
        a = [p] * 12 if ptrs is None else ptrs[:12]
        o = [p] * 8 if ptrs is None else ptrs[12:]
        return lib.sgpr_pairs_train_backward(*a, wn, wp, g, f, t, h, *o, ws, wb, None)

    for call, nptr in ((fwd, 12), (bwd, 20)):
        for k in range(nptr):
            ptrs = [p] * nptr
            ptrs[k] = None
            assert call(ptrs=ptrs) == -1 and b"NULL" in lib.sgpr_last_error(), k
        for g in (0, -1, 1025):
            assert call(g=g) == -2 and b"G" in lib.sgpr_last_error()
        assert call(f=129) == -2 and call(f=0) == -2
        assert call(t=65) == -2 and call(t=0) == -2
        assert call(h=65) == -2 and call(h=0) == -2
        assert call(wb=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
        assert call(ws=None) == -7
        assert call(wn=-1.0) == -1 and call(wp=float("nan")) == -1


def test_workspace_bound():
    from sg_pr_amd import engine
    lib = engine.load_library()
    ws = lib.sgpr_pairs_train_workspace_bytes
    prev = 0
    for g in (1, 2, 37, 255, 256, 257, 1000, 1024):
        cur = ws(g, 32, 16, 16)
        assert cur >= prev and cur > 0, g
        prev = cur
    assert ws(256, 32, 16, 16) <= 16 * 2 ** 20
    assert ws(1024, 32, 16, 16) < 1024 * 1024 * 32 * 4
    assert ws(1024, 128, 64, 64) > 0
    for bad in ((0, 32, 16, 16), (1025, 32, 16, 16), (4, 129, 16, 16), (4, 32, 65, 16), (4, 32, 16, 65)):
        assert ws(*bad) == 0


# ---------------------------------------------------------------------------------------------------- pair_classes
def _world():
    from sg_pr_amd import synth
    c, l, _, poses = synth.world_sequence(num_graphs=90, node_num=100, seed=5)
    return c, l, poses


def test_pair_classes_is_target_of_entry_for_entry():
    from sg_pr_amd.train import PairSet, pair_classes
    _, _, poses = _world()
    xz = np.ascontiguousarray(poses[:, [3, 11]], dtype=np.float64)
    ids = np.arange(90)
    cls = pair_classes(xz, ids)
    assert cls.dtype == np.uint8 and cls.shape == (90, 90)
    assert (np.diag(cls) == 2).all()
    i, j = np.nonzero(cls <= 1)
    assert len(i) > 0 and (cls == 0).any() and (cls == 1).any() and (cls == 2).sum() > 90
    want = PairSet._targets(xz, np.stack((i, j), axis=1), 3.0)
    assert np.array_equal(want, cls[i, j].astype(np.float32))
    # everything else off the diagonal is where target_of would stop the run
    d = np.sqrt(((xz[:, None] - xz[None]) ** 2).sum(-1))
    skipped = (cls == 2) & ~np.eye(90, dtype=bool)
    assert ((d[skipped] > 3.0) & (d[skipped] < 20.0)).all()
    # batches cut as SGFitter cuts them hold all three classes
    sub = pair_classes(xz, np.array([3, 4, 50, 3]))
    assert sub.shape == (4, 4) and sub[0, 3] == 1 and sub[3, 0] == 1      # a repeated scan: distance 0
    assert np.array_equal(sub[:3, :3], cls[np.ix_([3, 4, 50], [3, 4, 50])])


def test_pair_classes_thresholds_and_sequences():
    from sg_pr_amd.train import pair_classes
    xz = np.array([[0.0, 0.0], [1.8, 2.4], [12.0, 16.0], [1.8, 2.4000001], [12.0, 15.999999]])
    cls = pair_classes(xz, np.arange(5), p_thresh=3.0)
    assert cls[0, 1] == 1 and cls[1, 0] == 1           # exactly 3.0: positive
    assert cls[0, 2] == 0 and cls[2, 0] == 0           # exactly 20.0: negative
    assert cls[0, 3] == 2 and cls[0, 4] == 2
    seq = np.array([0, 1, 0, 0, 1])
    cls = pair_classes(xz, np.arange(5), sequence=seq)
    assert cls[0, 1] == 2 and cls[1, 0] == 2 and cls[0, 2] == 0
    assert cls[2, 4] == 2 and cls[4, 2] == 2          # a micrometre apart, but in different frames
    assert pair_classes(xz, np.arange(5))[2, 4] == 1
    assert (np.diag(cls) == 2).all()
    assert pair_classes(xz, [0, 1], p_thresh=2.9)[0, 1] == 2
    assert pair_classes(xz, [0, 2], d_neg=20.5)[0, 1] == 2


# ---------------------------------------------------------------------------------------------------- augment
def _augment_today(centers, generator):
    """sg_pr_amd.train.augment as it was before shared_flip existed (kept here to pin the default)."""
    from sg_pr_amd.train import _rot_x, _rot_y, _rot_z
    g, n, _ = centers.shape
    b = g // 2
    dev = centers.device
    x = centers.to(torch.float64)

    def rand(*shape):
        return torch.rand(*shape, generator=generator, device=dev, dtype=torch.float64)

    def randn(*shape):
        return torch.randn(*shape, generator=generator, device=dev, dtype=torch.float64)

    flip = rand(b) > 0.5
    flip = torch.cat((flip, flip))
    x = torch.cat((torch.where(flip.view(g, 1, 1), -x[..., :1], x[..., :1]), x[..., 1:]), dim=2)
    x = torch.bmm(x, _rot_z(rand(g) * (2.0 * math.pi))).to(torch.float32).to(torch.float64)
    x = x + torch.clamp(0.01 * randn(g, n, 3), -0.05, 0.05)
    x = x * (0.8 + 0.45 * rand(g)).view(g, 1, 1)
    ang = torch.clamp(0.015 * randn(g, 3), -0.045, 0.045)
    r = torch.bmm(_rot_z(ang[:, 2]), torch.bmm(_rot_y(ang[:, 1]), _rot_x(ang[:, 0])))
    x = torch.bmm(x, r).to(torch.float32).to(torch.float64)
    x = x + (rand(g, 1, 3) * 0.6 - 0.3)
    return x.to(torch.float32)


def test_augment_default_is_unchanged():
    from sg_pr_amd.train import augment
    c, _, _ = _world()
    centers = torch.from_numpy(c[:16])
    for seed in range(3):
        g1, g2, g3 = (torch.Generator().manual_seed(seed) for _ in range(3))
        want = _augment_today(centers, g1)
        assert torch.equal(augment(centers, g2), want)
        assert torch.equal(augment(centers, g3, shared_flip=False), want)


def test_shared_flip_mirrors_all_graphs_or_none():
    from sg_pr_amd.train import augment
    # four well-separated points per graph: the sign of the triple product survives rotation, scale > 0 and a 0.05 jitter
    base = torch.tensor([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0], [0.0, 0.0, 10.0]])
    centers = base.unsqueeze(0).repeat(12, 1, 1).contiguous()

    def handed(x):
        x = x.double()
        return torch.sign(torch.det(torch.stack((x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]), dim=1)))

    assert (handed(centers) == 1).all()
    seen = set()
    mixed_default = False
    for seed in range(20):
        s = handed(augment(centers, torch.Generator().manual_seed(seed), shared_flip=True))
        assert (s == s[0]).all() and float(s[0]) != 0.0, seed
        seen.add(float(s[0]))
        d = handed(augment(centers, torch.Generator().manual_seed(seed)))
        assert torch.equal(d[:6], d[6:])                  # the default: one draw per listed pair
        mixed_default = mixed_default or bool((d != d[0]).any())
    assert seen == {1.0, -1.0}
    assert mixed_default


# ---------------------------------------------------------------------------------------------------- the reference
def test_reference_formulation_agrees_with_gathered_bce(oracle_sd):
    import train_pairs_ref as ref
    from sg_pr_amd.parser_sg import sgpr_args
    from sg_pr_amd.sg_net import SG
    model = SG(sgpr_args(), 12)
    model.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in oracle_sd.items()})
    model = model.double()
    rng = np.random.default_rng(0)
    g = 23
    rep0 = torch.from_numpy(rng.normal(0.0, 2.0, size=(g, 32)))
    cls = torch.from_numpy(rng.integers(0, 3, size=(g, g)).astype(np.uint8))
    names = ref.PARAMS
    for w_neg, w_pos in ((1.0, 1.0), (0.5, 3.0)):
        rep_a = rep0.clone().requires_grad_(True)
        p = {n: dict(model.named_parameters())[n].detach().clone().requires_grad_(True) for n in names}
        loss_a, pred_a, wsum = ref.ref_pairs_loss(rep_a, cls, p, w_neg, w_pos, chunk=7, backward=True)
        rep_b = rep0.clone().requires_grad_(True)
        model.zero_grad(set_to_none=True)
        loss_b, pred_b, (i, j) = ref.gathered_pairs_loss(rep_b, cls, model, w_neg, w_pos)
        loss_b.backward()
        assert abs(float(loss_a) - float(loss_b)) <= 1e-12 * max(1.0, abs(float(loss_b)))
        assert float((pred_a[i, j] - pred_b).abs().max()) <= 1e-13
        assert abs(float(wsum) - (w_neg * int((cls == 0).sum()) + w_pos * int((cls == 1).sum()))) <= 1e-9
        assert float((rep_a.grad - rep_b.grad).norm()) <= 1e-11 * float(rep_b.grad.norm())
        for n in names:
            want = dict(model.named_parameters())[n].grad
            assert float((p[n].grad - want).norm()) <= 1e-11 * max(float(want.norm()), 1e-30), n
    # no labelled pair: loss 0, gradients 0, nothing NaN
    rep_a = rep0.clone().requires_grad_(True)
    p = {n: dict(model.named_parameters())[n].detach().clone().requires_grad_(True) for n in names}
    loss, pred, wsum = ref.ref_pairs_loss(rep_a, torch.full((g, g), 2, dtype=torch.uint8), p, backward=True)
    assert float(loss) == 0.0 and float(wsum) == 0.0 and torch.isfinite(pred).all()
    assert float(rep_a.grad.abs().max()) == 0.0


def test_cli_and_fitter_arguments():
    import inspect
    from sg_pr_amd.train import SGFitter, parse_cli
    assert parse_cli([]).in_batch == "off"
    assert parse_cli(["cfg.yml", "--in-batch", "balanced", "--hard-negatives", "2"]).in_batch == "balanced"
    with pytest.raises(SystemExit):
        parse_cli(["--in-batch", "some"])
    assert inspect.signature(SGFitter.__init__).parameters["in_batch"].default == "off"
