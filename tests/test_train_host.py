"""Host side of sg_pr_amd.train (no GPU): augmentation, pair lists and targets, batching, checkpoint layout, CLI."""
import math
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def _graphs(b=64, n=100, n_real=60, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.zeros(2 * b, n, 3)
    c[:, :n_real] = torch.rand(2 * b, n_real, 3, generator=g) * 40 - 20
    return c


def test_augment_is_seeded_and_moves_padded_slots():
    from sg_pr_amd.train import augment
    c = _graphs()
    a1 = augment(c, torch.Generator().manual_seed(5))
    a2 = augment(c, torch.Generator().manual_seed(5))
    a3 = augment(c, torch.Generator().manual_seed(6))
    assert a1.dtype == torch.float32 and a1.shape == c.shape
    assert torch.equal(a1, a2) and not torch.equal(a1, a3)
    assert float(a1[:, 60:].abs().max()) > 0.0           # padded slots (centre 0) are transformed too
    assert float(a1[:, 60:].abs().max()) < 1.0           # ... but only by jitter, perturbation and shift


def test_augment_preserves_geometry_up_to_the_documented_noise():
    """Without jitter the map is x -> s (flip x) Rz R' + t: distances scale by s in [0.8, 1.25], heights (z) change only
    by the small-angle perturbation, and the pair's two graphs share the flip."""
    from sg_pr_amd import train
    b, n = 256, 50
    c = _graphs(b, n, n)
    gen = torch.Generator().manual_seed(1)
    out = train.augment(c, gen).double()
    cd = c.double()
    d_in = torch.cdist(cd, cd)
    d_out = torch.cdist(out, out)
    ratio = (d_out[:, 0, 1:] / d_in[:, 0, 1:])
    # jitter is <= 0.05 per coordinate -> <= 0.2 on a distance of >= a few metres
    scale = ratio.median(dim=1).values
    assert float(scale.min()) >= 0.79 and float(scale.max()) <= 1.26
    assert float(scale.std()) > 0.05                       # the scale is drawn per graph
    # orientation of the xy plane: the determinant of the fitted 2D linear map gives the flip (shared by a pair)
    x_in = cd[..., :2] - cd[..., :2].mean(1, keepdim=True)
    x_out = out[..., :2] - out[..., :2].mean(1, keepdim=True)
    m = torch.linalg.lstsq(x_in, x_out).solution
    det = torch.linalg.det(m)
    flips = det < 0
    assert torch.equal(flips[:b], flips[b:])
    frac = float(flips[:b].double().mean())
    assert 0.3 < frac < 0.7
    # z: a rotation about z plus angles <= 0.045 rad: heights move by at most 0.045 * |xy| * 1.25 + jitter + shift
    dz = (out[..., 2] - out[..., 2].mean(1, keepdim=True)) / scale.view(-1, 1) - \
        (cd[..., 2] - cd[..., 2].mean(1, keepdim=True))
    bound = 0.064 * cd[..., :2].norm(dim=-1).max() + 0.15
    assert float(dz.abs().max()) <= float(bound)
    # the rotation about z is uniform: the fitted angle (flip removed) spreads over the circle
    ang = torch.atan2(m[:, 0, 1] * torch.where(flips, -1.0, 1.0).double(), m[:, 0, 0])
    hist = torch.histc(ang.float(), bins=4, min=-math.pi, max=math.pi)
    assert float(hist.min()) >= 0.12 * len(ang)


def test_augment_shift_and_jitter_bounds():
    from sg_pr_amd import train
    # a single point at the origin in every slot: rotations do nothing, so out = s * (jitter) R' + shift
    c = torch.zeros(4096, 2, 3)
    out = train.augment(c, torch.Generator().manual_seed(2)).double()
    shift = out.mean(1)
    assert float(shift.abs().max()) <= 0.3 + 1.25 * 0.05 * math.sqrt(3) + 1e-6
    spread = (out[:, 0] - out[:, 1]).abs()
    assert float(spread.max()) <= 2 * 1.25 * 0.05 * math.sqrt(3) + 1e-6
    assert 0.005 < float(spread.std()) < 0.03


def test_pair_lists_targets_and_exit_rule(tmp_path):
    from sg_pr_amd.parser_sg import sgpr_args
    from sg_pr_amd.train import PairSet, target_of
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "00.txt").write_text("0.json 3.json\n0.json 250.json\n3.json 250.json\n")
    (lists / "08.txt").write_text("250.json 3.json\n")
    a = sgpr_args()
    a.pair_list_dir, a.graph_pairs_dir = str(lists), os.path.join(GOLDEN, "data")
    a.train_sequences, a.eval_sequences = ["00"], ["08"]
    data = PairSet.from_files(a)
    assert len(data.labels) == 3                          # every graph packed once
    assert data.centers.shape == (3, 100, 3)
    assert data.train_pairs.tolist() == [[0, 1], [0, 2], [1, 2]]
    assert data.eval_pairs.tolist() == [[2, 1]]
    assert data.train_targets.tolist() == [1.0, 0.0, 0.0] and data.eval_targets.tolist() == [0.0]
    assert target_of(3.0, 3) == 1.0 and target_of(20.0, 3) == 0.0
    with pytest.raises(SystemExit):
        target_of(10.0, 3)
    poses = np.zeros((2, 12))
    poses[1, 3] = 5.0
    with pytest.raises(SystemExit):
        PairSet(np.zeros((2, 4, 3)), -np.ones((2, 4)), poses, [[0, 1]], [])
    with pytest.raises(ValueError):
        PairSet(np.zeros((2, 4, 3)), -np.ones((2, 4)), poses, [[0, 2]], [])


def test_batches_cover_every_pair_once():
    from sg_pr_amd.train import batches_of
    rng = np.random.default_rng(0)
    b = batches_of(300, 128, rng)
    assert [len(x) for x in b] == [128, 128, 44]
    assert sorted(np.concatenate(b).tolist()) == list(range(300))
    assert not np.array_equal(np.concatenate(b), np.arange(300))
    b2 = batches_of(300, 128, np.random.default_rng(0))
    assert all(np.array_equal(x, y) for x, y in zip(b, b2))


def test_dense_features_match_the_packed_graph():
    from sg_pr_amd import synth
    from sg_pr_amd.train import dense_features
    c, l, _ = synth.make_graphs(4, 64, 20, 50, 0)
    want = synth.dense_features(c, l)
    got = dense_features(torch.from_numpy(c), torch.from_numpy(l)).numpy()
    assert np.array_equal(got, want)


def test_checkpoint_key_layout_loads_both_ways(tmp_path):
    from collections import OrderedDict
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    from sg_pr_amd.train import checkpoint_state
    a = sgpr_args()
    torch.manual_seed(0)
    model = sg_net.SG(a, 12)
    sd = checkpoint_state(model)
    assert len(sd) == 50 and all(k.startswith("module.") for k in sd)
    path = str(tmp_path / "0.pth")
    torch.save(sd, path)
    loaded = torch.load(path, map_location="cpu")
    stripped = OrderedDict((k[7:], v) for k, v in loaded.items())          # the reference's loader (sg_net.py:166-173)
    fresh = sg_net.SG(a, 12)
    fresh.load_state_dict(stripped)
    a.model = path
    trainer = sg_net.SGTrainer(a, False)
    for k, v in model.state_dict().items():
        assert torch.equal(trainer.model.state_dict()[k], v)


def test_cli_parsing():
    from sg_pr_amd.train import parse_cli
    ns = parse_cli(["cfg.yml", "--epochs", "4", "--init", "m.pth", "--seed", "9"])
    assert (ns.config, ns.epochs, ns.init, ns.seed) == ("cfg.yml", 4, "m.pth", 9)
    ns = parse_cli([])
    assert (ns.config, ns.epochs, ns.init, ns.seed) == ("./config/config.yml", None, None, 0)


def test_inference_behaviour_unchanged():
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    with pytest.raises(NotImplementedError):
        sg_net.SGTrainer(sgpr_args(), True)
