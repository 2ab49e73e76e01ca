"""Hard-pair mining in training (SGFitter hard_negatives / hard_positives / mine_every) and in the evaluation CLI
(place_db --hard): mining off changes nothing, mined pairs follow PairSet's rule within one sequence and equal the
brute-force matrix of the current weights, runs are reproducible, and the log records the count."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_mine import _reference

pytestmark = pytest.mark.gpu


def _args(**kw):
    from sg_pr_amd.parser_sg import sgpr_args
    a = sgpr_args()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _data(n=90, seed=5, n_train=48):
    """Graphs of one synthetic world split into two sequences (ids 0 / 1 by index), base pairs within each."""
    from sg_pr_amd import synth
    from sg_pr_amd.train import PairSet
    c, l, _, poses = synth.world_sequence(num_graphs=n, node_num=100, seed=seed)
    xz = poses[:, [3, 11]]
    seq = (np.arange(n) >= n // 2).astype(np.int64)
    d = np.sqrt(((xz[:, None] - xz[None]) ** 2).sum(-1))
    i, j = np.triu_indices(n, 1)
    same = seq[i] == seq[j]
    pos = np.nonzero(same & (d[i, j] <= 3.0))[0]
    neg = np.nonzero(same & (d[i, j] >= 20.0))[0]
    rng = np.random.default_rng(seed)
    pick = np.concatenate((pos[:n_train // 2], rng.choice(neg, size=n_train // 2, replace=False)))
    pairs = np.stack((i[pick], j[pick]), axis=1)
    return PairSet(c, l, poses, pairs, pairs[::3], sequence=seq)


def _fitter(tmp_path, seed=0, **kw):
    from sg_pr_amd.train import SGFitter
    return SGFitter(_args(batch_size=16, logdir=str(tmp_path), epochs=1), seed=seed, data=_data(), **kw)


def _state(f):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in f.model.state_dict().items()}


def _equal_states(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_mining_off_is_todays_fitter(tmp_path):
    from sg_pr_amd.train import batches_of
    states = []
    for kw in ({}, {"hard_negatives": 0, "hard_positives": 0, "mine_every": 1}):
        f = _fitter(tmp_path / str(len(states)), seed=11, **kw)
        for ids in (batches_of(len(f.data.train_pairs), 16, f.rng) * 2)[:5]:
            f.step(ids)
        states.append(_state(f))
    _equal_states(states[0], states[1])
    # a whole fit (mining epochs included, had mining been on): same batches, draws and state
    fits = []
    for kw in ({}, {"hard_negatives": 0, "hard_positives": 0, "mine_every": 1}):
        f = _fitter(tmp_path / ("fit%d" % len(fits)), seed=4, **kw).fit(epochs=3)
        assert f.last_mined is None
        fits.append((_state(f), f.rng.bit_generator.state, f.generator.get_state()))
    _equal_states(fits[0][0], fits[1][0])
    assert fits[0][1] == fits[1][1] and torch.equal(fits[0][2], fits[1][2])


def test_mined_pairs_follow_the_rule_and_the_matrix(tmp_path):
    from sg_pr_amd.train import NEG_DISTANCE, PairSet
    f = _fitter(tmp_path, seed=2, hard_negatives=4, hard_positives=2)
    bn = {k: v.clone() for k, v in f.model.state_dict().items() if "running" in k or "num_batches" in k}
    gen = f.generator.get_state()
    mined = f.mine()
    # no BatchNorm statistic moved, no draw from the generator, the model is back in training mode
    for k, v in f.model.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert torch.equal(f.generator.get_state(), gen) and f.model.training
    data = f.data
    pairs, targets = mined["pairs"], mined["targets"]
    assert len(pairs) > 0 and set(np.unique(targets).tolist()) <= {0.0, 1.0}
    assert np.array_equal(targets, PairSet._targets(data.xz, pairs, data.p_thresh))
    assert (data.sequence[pairs[:, 0]] == data.sequence[pairs[:, 1]]).all()            # within one sequence
    assert (pairs[:, 0] < pairs[:, 1]).all() and len(np.unique(pairs, axis=0)) == len(pairs)
    base = {tuple(sorted(p)) for p in data.train_pairs.tolist()}
    assert not any(tuple(p) in base for p in pairs.tolist())
    d = np.sqrt(((data.xz[pairs[:, 0]] - data.xz[pairs[:, 1]]) ** 2).sum(1))
    assert ((d <= data.p_thresh) | (d >= NEG_DISTANCE)).all()
    # every row's mined columns: the brute-force matrix of the current weights, masked and sorted
    f.model.eval()
    eng = f.model.engine()
    kinds = set()
    for sid, members, positives, vals, idx in mined["lists"]:
        assert (data.sequence[members] == sid).all()
        assert set(members.tolist()) <= set(np.unique(data.train_pairs).tolist())
        g = torch.from_numpy(members).cuda()
        with torch.no_grad():
            pooled = f.model.embed(f.centers[g], f.labels[g])[0]
        score = eng.score_all_pairs(pooled, pooled).cpu().numpy()
        k = idx.shape[1]
        wv, wi = _reference(score, data.xz[members], k, positives, d_pos=data.p_thresh, d_neg=NEG_DISTANCE)
        assert np.array_equal(idx, wi), (sid, positives)
        assert np.array_equal(vals.view(np.uint32), wv.view(np.uint32)), (sid, positives)
        kinds.add((sid, positives))
    f.model.train()
    assert kinds == {(0, False), (0, True), (1, False), (1, True)}


def test_mining_epochs_are_reproducible_and_logged(tmp_path):
    runs = []
    for r in range(2):
        logdir = tmp_path / ("run%d" % r)
        f = _fitter(logdir, seed=7, hard_negatives=2, hard_positives=1, mine_every=1)
        f.fit(epochs=2)                                   # epoch 1 mines (e >= mine_every, e % mine_every == 0)
        runs.append((f.last_mined, _state(f)))
        recs = [json.loads(line) for line in open(os.path.join(str(logdir), f.LOG_NAME))]
        mine_recs = [x for x in recs if "mined_pairs" in x]
        assert [x["epoch"] for x in mine_recs] == [1]
        assert mine_recs[0]["mined_pairs"] == len(f.last_mined["pairs"]) > 0
        assert mine_recs[0]["mined_negatives"] + mine_recs[0]["mined_positives"] == mine_recs[0]["mined_pairs"]
        assert mine_recs[0]["mine_seconds"] > 0
        # epoch 1 trained on base + mined pairs
        seen = [x["pairs"] for x in recs if x.get("epoch") == 1 and "pairs" in x]
        assert seen[-1] == len(f.data.train_pairs) + len(f.last_mined["pairs"])
    (m0, s0), (m1, s1) = runs
    assert np.array_equal(m0["pairs"], m1["pairs"]) and np.array_equal(m0["targets"], m1["targets"])
    for a, b in zip(m0["lists"], m1["lists"]):
        assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))
    _equal_states(s0, s1)


def test_place_db_cli_hard(tmp_path, ckpt_path):
    from sg_pr_amd import graph_store, place_db, synth
    from sg_pr_amd.parser_sg import sgpr_args
    from sg_pr_amd.sg_net import SGTrainer
    n = 600
    centers, labels, _, poses = synth.world_sequence(n, 100, seed=12)
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
    place_db.main([str(cfg), "--k", "1", "--window", "50", "--hard", "4"])
    z = np.load(tmp_path / "eva" / "07_hard.npz")
    for key in ("neg_indices", "neg_scores", "pos_indices", "pos_scores"):
        assert z[key].shape == (n, 4), key
    # against the matrix of the same model: score_all_pairs, masked and sorted
    args = sgpr_args()
    args.model = ckpt_path
    model = SGTrainer(args, False).model.eval()
    db = place_db.PlaceDatabase(model, capacity=n)
    db.add(seq.centers, seq.labels)
    score = model.engine().score_all_pairs(db.pooled, db.pooled).cpu().numpy()
    xz = poses[:, [3, 11]]
    for pos, key in ((False, "neg"), (True, "pos")):
        wv, wi = _reference(score, xz, 4, pos, window=50)
        assert np.array_equal(z[key + "_indices"], wi), key
        assert np.array_equal(z[key + "_scores"].view(np.uint32), wv.view(np.uint32)), key
    assert (z["pos_indices"][:, 0] >= 0).sum() > 0
    # the count the CLI prints: hardest negative above the best positive (exact where a frame has < 4 positives)
    best = np.where(z["pos_indices"] >= 0, z["pos_scores"], -np.inf).max(1)
    want = (z["neg_indices"][:, 0] >= 0) & (z["pos_indices"][:, 0] >= 0) & (z["neg_scores"][:, 0] > best)
    assert np.array_equal(z["neg_above_pos"], want)
    assert np.array_equal(z["exact"], z["pos_indices"][:, -1] < 0)
