"""Plain-torch formulation of the all-pairs training tail (sg_pr_amd.train.pairs_tail), written from train_ref.forward_pair's
pieces: tensor network + fully_connected_first + scoring_layer over every ordered pair of rep [G,F], and the weighted
BCE over the labelled ones.  Any device and dtype: float64 on the CPU is the checker of the HIP op, float32 on the GPU
its yardstick and memory baseline.  Rows are walked in chunks so that G = 1024 fits."""
import torch
import torch.nn.functional as Fn

PARAMS = ("tensor_network.weight_matrix", "tensor_network.weight_matrix_block", "tensor_network.bias",
          "fully_connected_first.weight", "fully_connected_first.bias", "scoring_layer.weight", "scoring_layer.bias")


def pairs_pred(rep, p, rows=slice(None)):
    """pred [R,G] for the row graphs rep[rows] against every graph of rep [G,F]; p: the seven tensors by PARAMS' names."""
    w, v = p[PARAMS[0]], p[PARAMS[1]]
    f = w.shape[0]
    e1 = rep[rows]
    a = torch.einsum("rf,fgt->rgt", e1, w)
    s = torch.einsum("rgt,jg->rjt", a, rep)
    s = s + torch.matmul(e1, v[:, :f].t()).unsqueeze(1) + torch.matmul(rep, v[:, f:].t()).unsqueeze(0) + \
        p[PARAMS[2]].reshape(1, 1, -1)
    z = torch.relu(s)
    h = torch.relu(Fn.linear(z, p[PARAMS[3]], p[PARAMS[4]]))
    return torch.sigmoid(Fn.linear(h, p[PARAMS[5]], p[PARAMS[6]])).squeeze(-1)


def pair_weights(cls, w_neg, w_pos, dtype):
    cls = cls.long()
    return (cls == 0).to(dtype) * w_neg + (cls == 1).to(dtype) * w_pos


def _bce_sum(pred, y, w):
    """Fn.binary_cross_entropy(pred, y, weight=w, reduction="sum"), written out for a pred that holds a NaN: torch's CPU
    kernel refuses one ("all elements of input should be between 0 and 1"), its formula - the logs clamped at -100 by
    torch.clamp, which keeps a NaN, times the weight - hands it on, as its GPU kernel does."""
    if bool(torch.isnan(pred).any()):
        return -(w * (y * torch.log(pred).clamp(min=-100.0) + (1.0 - y) * torch.log1p(-pred).clamp(min=-100.0))).sum()
    return Fn.binary_cross_entropy(pred, y, weight=w, reduction="sum")


def ref_pairs_loss(rep, cls, p, w_neg=1.0, w_pos=1.0, chunk=128, backward=False):
    """-> (loss = sum w l / sum w, pred [G,G], wsum).  backward=True also runs loss.backward() chunk by chunk (the
    gradients land in rep.grad and the parameters' .grad; the returned loss is then detached)."""
    g = rep.shape[0]
    w = pair_weights(cls.to(rep.device), w_neg, w_pos, rep.dtype)
    y = (cls.to(rep.device).long() == 1).to(rep.dtype)
    wsum = w.sum()
    scale = 1.0 / wsum if float(wsum) > 0 else 0.0
    total = torch.zeros((), dtype=rep.dtype, device=rep.device)
    preds = []
    for r0 in range(0, g, chunk):
        rows = slice(r0, min(r0 + chunk, g))
        pred = pairs_pred(rep, p, rows)
        part = _bce_sum(pred, y[rows], w[rows]) * scale
        if backward:
            part.backward()
            part = part.detach()
        total = total + part
        preds.append(pred.detach())
    return total, torch.cat(preds), wsum


def gathered_pairs_loss(rep, cls, model, w_neg=1.0, w_pos=1.0):
    """The same loss the way torch ops would train on it: gather the labelled pairs to [P,F,1], sg_pr_amd.train's
    tensor_network and head, weighted mean BCE.  -> (loss, pred [P], (i, j) index tensors)."""
    from sg_pr_amd import train
    i, j = torch.nonzero(cls.to(rep.device).long() <= 1, as_tuple=True)
    y = (cls.to(rep.device).long()[i, j] == 1).to(rep.dtype)
    w = torch.where(y > 0, torch.full_like(y, w_pos), torch.full_like(y, w_neg))
    pred = train.head(model, train.tensor_network(model.tensor_network, rep[i].unsqueeze(-1), rep[j].unsqueeze(-1)))
    if len(i) == 0 or float(w.sum()) == 0:
        return pred.sum() * 0.0, pred, (i, j)
    return Fn.binary_cross_entropy(pred, y, weight=w, reduction="sum") / w.sum(), pred, (i, j)
