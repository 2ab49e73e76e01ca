"""The all-pairs training tail (sg_pr_amd.train.PairsTail, csrc/sgpr_train_pairs.hip) on a pooled vector that is not finite -
what a diverged embedding hands it - against tests/train_pairs_ref.py in float64: the loss must say so.

G = 37 golden pooled vectors, graph 11 planted (whole vector NaN; one NaN element; one +inf element), the labels of
test_gpu_train_pairs._random_cls.  torch's tail (torch.relu, F.binary_cross_entropy) gives a NaN loss there; a ReLU
written fmaxf(a, 0) gives relu(NaN) = 0, a finite pred, a finite loss and no gradient from those pairs, and training
goes on.  Required:
  pred is NaN exactly on that graph's row and column (NaN plants), every other entry has the clean call's bits (a row
  owner's other pairs do not read the planted vector); the +inf plant is held to the one-sided rule of
  tests/nonfinite_ref.py: NaN, or within 1e-4 of the float64 pred (test_gpu_train_pairs' bar on pred, here per entry:
  preds lie in [0, 1]) where that is not NaN;
  a labelled pair of the planted graph: the loss is NaN and each of the eight gradients holds a non-finite value, so
  that no optimizer step passes silently;
  every pair of the planted graph unlabelled (cls 2): the loss has the clean call's bits;
  a NaN in a parameter (fc1_b, one element of W): the loss is NaN.
Found on an MI355X in the unlabelled case (recorded, as the finish kernel multiplies a zero dA by the NaN vector): see
test_unlabelled_pairs_of_the_planted_graph's docstring."""
import numpy as np
import pytest
import torch

import nonfinite_ref as nf
import train_pairs_ref as ref
from test_gpu_train_pairs import GRADS, _pooled, _random_cls, _run_op, _tail_params

pytestmark = pytest.mark.gpu

G, P = 37, 11
PRED_BAR = 1e-4
PLANTS = ["NaN vector", "one NaN element", "one +inf element"]


def _planted(rep, plant):
    x = rep.detach().cpu().float().contiguous().clone()
    a = x.numpy()
    if plant == "NaN vector":
        nf.plant_bits(a, (P, slice(None)), nf.QNAN_POS)
    elif plant == "one NaN element":
        nf.plant_bits(a, (P, 16), nf.QNAN_NEG)
    else:
        a[P, 15] = np.inf
    return x


def _touch_mask():
    m = torch.zeros(G, G, dtype=torch.bool)
    m[P], m[:, P] = True, True
    return m


def _ref64(rep, cls, params, w_neg, w_pos):
    p = {n: params[n].double() for n in ref.PARAMS}
    with torch.no_grad():
        loss, pred, _ = ref.ref_pairs_loss(rep.double(), cls, p, w_neg, w_pos)
    return float(loss), pred


@pytest.fixture(scope="module")
def clean(oracle_sd):
    rep = _pooled("golden", oracle_sd)[:G].detach().cpu().clone()
    params = _tail_params(oracle_sd)
    cls = _random_cls(G, G)
    assert int((cls[P] <= 1).sum()) > 0 and int((cls[:, P] <= 1).sum()) > 0      # the planted graph has labelled pairs
    op = _run_op(rep, cls, params, 1.0, 2.5)
    assert np.isfinite(float(op[0])) and torch.isfinite(op[1]).all() and all(torch.isfinite(x).all() for x in op[3])
    return rep, params, cls, op


def _check_pred(plant, pred, pred_clean, pred_ref):
    touch = _touch_mask()
    pred, pred_clean = pred.cpu(), pred_clean.cpu()
    assert torch.equal(pred[~touch], pred_clean[~touch]), (plant, "a pair of two healthy graphs changed bits")
    if "NaN" in plant:
        assert torch.isnan(pred_ref[touch]).all()                                # (the reference agrees: not vacuous)
        assert torch.equal(torch.isnan(pred), touch), (plant, "pred NaN pattern", int(torch.isnan(pred).sum()),
                                                       int(touch.sum()))
    else:
        owed = touch & ~torch.isnan(pred_ref)
        d = (pred.double() - pred_ref)[owed & ~torch.isnan(pred)].abs()
        print(plant, "reference NaN on %d of %d pairs of the graph, op NaN on %d; max |d| where both finite %.3g"
              % (int(torch.isnan(pred_ref[touch]).sum()), int(touch.sum()), int(torch.isnan(pred[touch]).sum()),
                 float(d.max()) if d.numel() else 0.0))
        assert d.numel() == 0 or float(d.max()) <= PRED_BAR, (plant, float(d.max()))


@pytest.mark.parametrize("plant", PLANTS)
def test_labelled_pairs_of_the_planted_graph(clean, plant):
    rep, params, cls, op_clean = clean
    x = _planted(rep, plant)
    loss_ref, pred_ref = _ref64(x, cls, params, 1.0, 2.5)
    loss, pred, wsum, grads = _run_op(x, cls, params, 1.0, 2.5)
    _check_pred(plant, pred, op_clean[1], pred_ref)
    status = {n: bool(torch.isfinite(g).all()) for n, g in zip(GRADS, grads)}
    print(plant, "loss", float(loss), "float64", loss_ref, "gradients all finite:", status)
    assert float(wsum) == float(op_clean[2])
    if "NaN" in plant:
        assert np.isnan(loss_ref)
    if np.isnan(loss_ref):         # (the +inf plant: a NaN in float64 as well - infinite terms of both signs meet)
        assert np.isnan(float(loss)), (plant, "a finite loss on a non-finite pooled vector", float(loss))
        silent = [n for n, ok in status.items() if ok]
        assert not silent, (plant, "gradients without a non-finite value", silent)
    else:
        assert np.isnan(float(loss)) or abs(float(loss) - loss_ref) <= 1e-6 * max(1.0, abs(loss_ref)), (plant, float(loss))


@pytest.mark.parametrize("plant", PLANTS[:2])
def test_unlabelled_pairs_of_the_planted_graph(clean, plant):
    """Every pair of the planted graph has cls 2: the loss is the clean call's, bit for bit.  The gradients, as found on
    an MI355X (printed by this test): d_b, d_fc1_b and d_fc2_b are finite with the clean call's bits - the planted pairs
    add a zero dlogit to them -; d_rep, d_W, d_V, d_fc1_w and d_fc2_w hold NaN: their sums multiply that zero by the NaN
    vector (dA = e_x dz in the row pass, dW = e_i dA in the finish kernel) or by the NaN activations (d_fc1_w = dh z,
    d_fc2_w = dlogit h).  torch's tail gives NaN there as well (its weight 0 times a NaN loss term is NaN, which the
    op's `cls <= 1` branch never forms)."""
    rep, params, cls, _ = clean
    cls2 = cls.clone()
    cls2[P], cls2[:, P] = 2, 2
    base = _run_op(rep, cls2, params, 1.0, 2.5)
    x = _planted(rep, plant)
    loss, pred, wsum, grads = _run_op(x, cls2, params, 1.0, 2.5)
    assert torch.equal(loss.reshape(1).view(torch.int32), base[0].reshape(1).view(torch.int32)), (float(loss), float(base[0]))
    assert float(wsum) == float(base[2])
    assert torch.equal(torch.isnan(pred).cpu(), _touch_mask())
    assert torch.equal(pred.cpu()[~_touch_mask()], base[1].cpu()[~_touch_mask()])
    status = {n: ("finite, clean bits" if torch.equal(g, b) else "finite") if torch.isfinite(g).all() else "non-finite"
              for n, g, b in zip(GRADS, grads, base[3])}
    print(plant, "unlabelled: gradients", status)
    for n in ("b", "fc1_b", "fc2_b"):
        assert status[n] == "finite, clean bits", (plant, n, status[n])


@pytest.mark.parametrize("which", ["fc1_b", "W"])
def test_nan_in_a_parameter(clean, which):
    rep, params, cls, _ = clean
    p = {k: v.clone() for k, v in params.items()}
    if which == "fc1_b":
        p["fully_connected_first.bias"].view(-1)[3] = float("nan")
    else:
        p["tensor_network.weight_matrix"][5, 7, 2] = float("nan")
    loss_ref, pred_ref = _ref64(rep, cls, p, 1.0, 2.5)
    assert np.isnan(loss_ref) and torch.isnan(pred_ref).all()
    loss, pred, _, _ = _run_op(rep, cls, p, 1.0, 2.5)
    assert torch.isnan(pred).all(), (which, int(torch.isnan(pred).sum()))
    assert np.isnan(float(loss)), (which, float(loss))
