"""One training step of sg_pr_amd.train (HIP EdgeConv op + torch) against the float64 formulation of the reference's
step (tests/train_ref.py), determinism, overfitting, checkpoints through the inference engine, and activation memory."""
import io
import os
import zipfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


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


def _model(sd):
    from sg_pr_amd.sg_net import SG
    m = SG(_args(), 12)
    m.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in sd.items()})
    return m.cuda().train()


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _step_vs_ref(sd):
    from sg_pr_amd.train import dense_features, train_loss
    import train_ref
    centers, labels = _golden_plus_synth(13)
    g = len(labels)                                  # 16 graphs: pairs (i, i + 8)
    feats = dense_features(torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda())
    target = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0], device="cuda")
    model = _model(sd)
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    loss, pred, lists = train_loss(model, feats, target)
    loss.backward()

    p = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point()) for k, v in before.items()}
    loss_r, pred_r, stats = train_ref.train_step_loss(p, feats.cpu().double(), target.cpu().double(),
                                                      [i.cpu() for i in lists])
    loss_r.backward()
    assert g == 16
    # fp32 step vs fp64: the loss to 1e-5 absolute, every gradient to 2e-3 of its norm (fp32 sums over 16 graphs x 1000
    # edges; a near-tie of the max edge that fp32 and fp64 break differently moves one node's gradient)
    assert abs(loss.item() - loss_r.item()) <= 1e-5, (loss.item(), loss_r.item())
    assert _relerr(pred, pred_r) <= 1e-4
    names = [n for n, _ in model.named_parameters()]
    assert len(names) + len(list(model.buffers())) == 50
    for name, prm in model.named_parameters():
        ref = p[name].grad
        assert prm.grad is not None and ref is not None, name
        if float(ref.norm()) == 0.0:
            assert float(prm.grad.abs().max()) <= 1e-6, name
            continue
        assert _relerr(prm.grad, ref) <= 2e-3, (name, _relerr(prm.grad, ref))
    want = train_ref.running_after({k: v for k, v in before.items() if "running" in k or "num_batches" in k}, stats)
    got = model.state_dict()
    for k, v in want.items():
        if "num_batches" in k:
            assert int(got[k]) == int(v), k
        else:
            assert _relerr(got[k], v) <= 1e-5, (k, _relerr(got[k], v))


def test_one_step_from_golden_model(oracle_sd):
    _step_vs_ref(oracle_sd)


def test_one_step_from_release_checkpoint(oracle):
    with zipfile.ZipFile(os.path.join(GOLDEN, "release_model.zip")) as z:
        name = sorted(n for n in z.namelist() if n.endswith("model.pth"))[0]
        sd = oracle.load_checkpoint(io.BytesIO(z.read(name)))
    _step_vs_ref(sd)


def _world(num_graphs=90, seed=5, p_thresh=3.0):
    """Graphs of one synthetic world and every pair (i, j), i < j, that is a positive (<= 3 m) or a negative (>= 20 m)."""
    from sg_pr_amd import synth
    c, l, _, poses = synth.world_sequence(num_graphs=num_graphs, node_num=100, seed=seed)
    xz = poses[:, [3, 11]]
    d = np.sqrt(((xz[:, None] - xz[None]) ** 2).sum(-1))
    i, j = np.triu_indices(num_graphs, 1)
    pos = np.nonzero(d[i, j] <= p_thresh)[0]
    neg = np.nonzero(d[i, j] >= 20.0)[0]
    rng = np.random.default_rng(seed)
    return c, l, poses, i, j, pos, rng.choice(neg, size=min(len(neg), len(pos)), replace=False)


def _fitter(tmp_path, seed=0, n_train=48, batch=16, augment=True, **kw):
    from sg_pr_amd.train import PairSet, SGFitter
    c, l, poses, i, j, pos, neg = _world()
    pick = np.concatenate((pos[:n_train // 2], neg[:n_train // 2]))
    pairs = np.stack((i[pick], j[pick]), axis=1)
    data = PairSet(c, l, poses, pairs, pairs[::3])
    f = SGFitter(_args(batch_size=batch, logdir=str(tmp_path), epochs=1, **kw), seed=seed, data=data)
    f.augment = augment
    return f


def test_same_seed_same_state_after_five_steps(tmp_path):
    from sg_pr_amd.train import batches_of
    sds = []
    for _ in range(2):
        f = _fitter(tmp_path, seed=11)
        for ids in (batches_of(len(f.data.train_pairs), 16, f.rng) * 2)[:5]:
            f.step(ids)
        torch.cuda.synchronize()
        sds.append({k: v.detach().cpu().clone() for k, v in f.model.state_dict().items()})
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k


def test_overfits_a_small_pair_list(tmp_path):
    # from scratch at lr 1e-4 (at the reference's 1e-3 a fresh model on these unnormalised coordinates saturates the
    # sigmoid within a few steps, where BCE's clamp leaves no gradient)
    f = _fitter(tmp_path, seed=3, n_train=32, batch=32, augment=False, learning_rate=1e-4)
    ids = np.arange(len(f.data.train_pairs))
    losses = [f.step(ids) for _ in range(60)]
    print("overfit losses", losses[0], losses[-1])
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])


def test_checkpoint_loads_into_inference_and_oracle(tmp_path, oracle):
    from sg_pr_amd import sg_net
    f = _fitter(tmp_path, seed=1)
    f.fit(epochs=1)
    path = os.path.join(str(tmp_path), "0.pth")
    assert os.path.exists(path) and os.path.exists(os.path.join(str(tmp_path), "0_best.pth"))
    sd_raw = torch.load(path, map_location="cpu")
    assert len(sd_raw) == 50 and all(k.startswith("module.") for k in sd_raw)
    log = open(os.path.join(str(tmp_path), "train_log.jsonl")).read().splitlines()
    assert any('"f1_max"' in line for line in log)
    args = _args(model=path)
    trainer = sg_net.SGTrainer(args, False)
    pairs = [[os.path.join(GOLDEN, "data", a + ".json"), os.path.join(GOLDEN, "data", b + ".json")]
             for a, b in (("0", "250"), ("0", "3"), ("250", "250"))]
    pred, gt = trainer.eval_batch_pair(pairs)
    sd = oracle.load_checkpoint(path)
    ref, gt_ref = oracle.eval_batch_pair(sd, pairs, args.node_num, args.K, args.p_thresh)
    assert float(np.max(np.abs(pred - ref))) <= 1e-4
    assert np.array_equal(gt, gt_ref)


def test_activation_memory_vs_dense_formulation(oracle_sd):
    from sg_pr_amd import synth
    from sg_pr_amd.train import dense_features, train_loss
    import train_ref
    c, l, _ = synth.make_graphs(256, 100, 20, 90, 0, kitti_like=True)
    feats = dense_features(torch.from_numpy(c).cuda(), torch.from_numpy(l).cuda())
    target = (torch.arange(128, device="cuda") % 2).float()
    model = _model(oracle_sd)
    _, _, lists = train_loss(model, feats, target, updates=0)
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def fused():
        loss, _, _ = train_loss(model, feats, target, updates=0)
        loss.backward()

    p = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}

    def dense():
        loss, _, _ = train_ref.train_step_loss(p, feats, target, lists)
        loss.backward()

    m_fused = peak(fused)
    model.zero_grad(set_to_none=True)
    m_dense = peak(dense)
    print("activation memory: fused %.1f MB, dense fp32 %.1f MB, ratio %.2f" % (m_fused / 2 ** 20, m_dense / 2 ** 20,
                                                                             m_dense / max(m_fused, 1)))
    assert m_fused * 3 <= m_dense
