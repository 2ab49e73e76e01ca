"""The float64 tail reference of tests/score_ref.py against the oracle (run in float64) and test_gpu_parity's
_tail_float64, and the checkpoint variants it builds: the same function where they promise it, a dead neuron that is dead,
a cancellation that cancels.  CPU only."""
import numpy as np
import pytest
import torch

import score_ref


def _inputs(seed, r=37, m=131, f=32, scale=4.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, scale, size=(r, f)).astype(np.float32), rng.normal(0, scale, size=(m, f)).astype(np.float32))


def _any_shape_sd():
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.filters_1, args.filters_2, args.filters_3, args.tensor_neurons, args.bottle_neck_neurons = 64, 64, 48, 16, 16
    torch.manual_seed(5)
    return {k: v.detach().clone() for k, v in sg_net.SG(args, 12).eval().state_dict().items()}


def _oracle64(oracle, sd, rows, cols):
    """oracle.score_all_pairs' pair expansion through oracle.score_from_pooled, every tensor in float64 (score_all_pairs
    itself stores into an fp32 matrix)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    r, m = rows.shape[0], cols.shape[0]
    a = torch.from_numpy(rows).double().repeat_interleave(m, dim=0)
    b = torch.from_numpy(cols).double().repeat(r, 1)
    return oracle.score_from_pooled(sd64, a, b).view(r, m).numpy()


def test_reference_matches_the_oracle_in_float64(oracle, oracle_sd):
    from test_gpu_parity import _tail_float64
    rows, cols = _inputs(1)
    ref = score_ref.tail(oracle_sd, rows, cols)
    want = _oracle64(oracle, oracle_sd, rows, cols)
    assert np.abs(ref["score"] - want).max() <= 1e-12
    assert np.abs(ref["score"] - _tail_float64(oracle_sd, rows, cols)).max() <= 1e-12
    # an any-shape architecture (F = 48): the oracle is shape-generic
    sd = _any_shape_sd()
    r2, c2 = _inputs(2, 17, 65, 48, 1.0)
    ref2 = score_ref.tail(sd, r2, c2)
    want2 = _oracle64(oracle, sd, r2, c2)
    assert np.abs(ref2["score"] - want2).max() <= 1e-12


def test_range_quantities_by_their_definitions(oracle_sd):
    rows, cols = _inputs(3, 5, 7)
    g = score_ref.gates(oracle_sd, rows, cols)
    w = oracle_sd["tensor_network.weight_matrix"].double().numpy()
    wb = oracle_sd["tensor_network.weight_matrix_block"].double().numpy()
    bias = oracle_sd["tensor_network.bias"].double().numpy().reshape(-1)
    am = um = l1 = 0.0
    for e1 in rows.astype(np.float64):
        for t in range(16):
            a = [sum(e1[i] * w[i, j, t] for i in range(32)) + wb[t, 32 + j] for j in range(32)]
            am, l1 = max(am, max(abs(x) for x in a)), max(l1, sum(abs(x) for x in a))
            um = max(um, abs(float(wb[t, :32] @ e1) + bias[t]))
    assert g["am"] == pytest.approx(am, rel=1e-12) and g["um"] == pytest.approx(um, rel=1e-12)
    assert g["l1"] == pytest.approx(l1, rel=1e-12) and g["em"] == float(np.abs(cols).max())
    assert score_ref.bound(g) == g["um"] + 32 * g["am"] * g["em"]


@pytest.mark.parametrize("which", ["tuned", "any-shape"])
def test_variants_are_what_they_claim(oracle_sd, which):
    sd = oracle_sd if which == "tuned" else _any_shape_sd()
    f = sd["tensor_network.weight_matrix"].shape[0]
    rows, cols = _inputs(4, 37, 131, f, 4.0 if which == "tuned" else 1.0)
    base = score_ref.tail(sd, rows, cols)
    for c in (0.125, 8.0):                         # the same function, exactly (float64 of the fp32 tensors)
        v = score_ref.reparametrised(sd, c)
        r = score_ref.tail(v, rows, cols)
        np.testing.assert_allclose(r["score"], base["score"], rtol=0, atol=1e-13)
        assert np.abs(score_ref.fold(v)).max() == pytest.approx(np.abs(score_ref.fold(sd)).max() / c, rel=1e-6)
    v, t, o = score_ref.dead_neuron_with_huge_fold(sd, [(rows, cols)])
    r = score_ref.tail(v, rows, cols)
    assert (r["h"][:, :, t] == 0.0).all()
    assert abs(score_ref.fold(v)[o, t]) == pytest.approx(1e5, rel=1e-6)
    v, t, t2, o = score_ref.live_cancellation(sd, [(rows, cols)])
    r = score_ref.tail(v, rows, cols)
    assert np.array_equal(r["h"][:, :, t], r["h"][:, :, t2]) and (r["h"][:, :, t] > 0).mean() > 0.2
    fv = score_ref.fold(v)
    assert 6e4 < abs(fv[o, t]) and 6e4 < abs(fv[o, t2])
