"""Plain-torch formulation of the reference's train-mode step (sg_net.py:79-138, 358-387; dgcnn.py:23-49), written from
the maths: the dense [B, 2C, N, k] edge tensor, Conv2d 1x1, BatchNorm with batch statistics, LeakyReLU, max over k,
and the two conv passes of process_batch (features_1 = [A; B], features_2 = [B; A]).  Any device and dtype: float64 on
the CPU is the checker of the fused HIP path; float32 on the GPU is the memory / time baseline.

The kNN lists are PASSED IN (the six lists of the HIP forward for the graphs [A; B]), so that near-ties of the
distances cannot send the two formulations down different graphs."""
import torch
import torch.nn.functional as Fn

BLOCKS = ("dgcnn_s_conv1", "dgcnn_s_conv2", "dgcnn_s_conv3", "dgcnn_f_conv1", "dgcnn_f_conv2", "dgcnn_f_conv3")


def edge_feature(x, idx):
    """get_graph_feature for given lists: x [B,C,N], idx [B,N,k] -> [B,2C,N,k] = cat(x_j - x_i, x_i), on x's device."""
    b, c, n = x.shape
    k = idx.shape[2]
    flat = (idx.to(x.device).long() + torch.arange(b, device=x.device).view(-1, 1, 1) * n).reshape(-1)
    xt = x.transpose(2, 1).reshape(b * n, c)
    nb = xt[flat].view(b, n, k, c)
    xi = xt.view(b, n, 1, c).expand(b, n, k, c)
    return torch.cat((nb - xi, xi), dim=3).permute(0, 3, 1, 2)


def edge_block(x, idx, w, gamma, beta, eps=1e-5):
    """Conv2d 1x1 (w [F, 2C]) -> BatchNorm2d (batch statistics) -> LeakyReLU(0.2) -> max over k.
    -> (y [B,F,N], batch mean [F], biased var [F])."""
    z = torch.einsum("fc,bcnk->bfnk", w, edge_feature(x, idx))
    mean = z.mean(dim=(0, 2, 3))
    var = z.var(dim=(0, 2, 3), unbiased=False)
    u = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * gamma.view(1, -1, 1, 1) + \
        beta.view(1, -1, 1, 1)
    return Fn.leaky_relu(u, 0.2).max(dim=-1)[0], mean, var


def pq_block(P, Q, idx, gamma, beta, eps=1e-5):
    """The same block from the per-node products: z[b,f,i,k] = P[b,f,idx[b,i,k]] + Q[b,f,i]."""
    b, f, n = P.shape
    k = idx.shape[2]
    g = idx.to(P.device).long().reshape(b, 1, n * k).expand(b, f, n * k)
    z = torch.gather(P, 2, g).view(b, f, n, k) + Q.unsqueeze(-1)
    mean = z.mean(dim=(0, 2, 3))
    var = z.var(dim=(0, 2, 3), unbiased=False)
    u = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * gamma.view(1, -1, 1, 1) + \
        beta.view(1, -1, 1, 1)
    return Fn.leaky_relu(u, 0.2).max(dim=-1)[0], mean, var


def pq_block_selected(P, Q, idx, gamma, beta, eps=1e-5):
    """pq_block with the op's documented choice of the max edge (include/sgpr.h), exact on ties.

    idx is clamped to [0, N).  The batch mean / biased var run over every one of the M = B N k edges.  The edge of
    (b, f, i) is chosen on P, not on the activation: the largest P for gamma >= 0, the smallest for gamma < 0 (gamma = 0
    selects as gamma > 0), the lowest k among equal P.  y is a gather at that k, so autograd sends dy to that edge only.
    -> (y [B,F,N], mean [F], biased var [F], sel [B,F,N] int64, s1 [B,F,N] = sum_k P[b,f,idx[b,i,k]])."""
    b, f, n = P.shape
    k = idx.shape[2]
    idx = idx.to(P.device).long().clamp(0, n - 1)
    g = idx.reshape(b, 1, n * k).expand(b, f, n * k)
    Pn = torch.gather(P, 2, g).view(b, f, n, k)
    z = Pn + Q.unsqueeze(-1)
    mean = z.mean(dim=(0, 2, 3))
    var = z.var(dim=(0, 2, 3), unbiased=False)
    key = torch.where(gamma.detach().view(1, -1, 1, 1) < 0, -Pn.detach(), Pn.detach())
    best = key.max(dim=-1, keepdim=True).values
    ks = torch.arange(k, device=P.device).view(1, 1, 1, k).expand_as(key)
    sel = torch.where(key == best, ks, k).min(dim=-1).values
    z_sel = torch.gather(z, 3, sel.unsqueeze(-1)).squeeze(-1)
    u = (z_sel - mean.view(1, -1, 1)) / torch.sqrt(var.view(1, -1, 1) + eps) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
    return Fn.leaky_relu(u, 0.2), mean, var, sel, Pn.detach().sum(dim=-1)


def conv_pass(p, feats, idx_lists, eps=1e-5):
    """dgcnn_conv_pass in train mode -> (emb [G,N,F3], {bn name: (mean, biased var, count)})."""
    stats = {}

    def branch(x, names, lists):
        for name, idx in zip(names, lists):
            w = p[name + ".0.weight"]
            x, m, v = edge_block(x, idx, w.reshape(w.shape[0], -1), p[name + ".1.weight"], p[name + ".1.bias"], eps)
            stats[name] = (m, v, x.shape[0] * x.shape[2] * idx.shape[2])
        return x

    xyz = branch(feats[:, :3, :], BLOCKS[:3], idx_lists[:3])
    sem = branch(feats[:, 3:, :], BLOCKS[3:], idx_lists[3:])
    x = torch.cat((xyz, sem), dim=1)
    w = p["dgcnn_conv_end.0.weight"]
    x = torch.matmul(w.reshape(w.shape[0], -1), x)
    m, v = x.mean(dim=(0, 2)), x.var(dim=(0, 2), unbiased=False)
    stats["dgcnn_conv_end"] = (m, v, x.shape[0] * x.shape[2])
    x = (x - m.view(1, -1, 1)) / torch.sqrt(v.view(1, -1, 1) + eps) * p["dgcnn_conv_end.1.weight"].view(1, -1, 1) + \
        p["dgcnn_conv_end.1.bias"].view(1, -1, 1)
    return Fn.leaky_relu(x, 0.2).permute(0, 2, 1), stats


def forward_pair(p, f1, f2, l1, l2):
    """SG.forward (sg_net.py:112-138) on two embedded sides -> score [B]."""
    def att(emb):
        ctx = torch.tanh(torch.mean(torch.matmul(emb, p["attention.weight_matrix"]), dim=1))
        s = torch.sigmoid(torch.matmul(emb, ctx.unsqueeze(-1)))
        return torch.matmul(emb.permute(0, 2, 1), s)

    e1, e2 = att(f1), att(f2)
    w = p["tensor_network.weight_matrix"]
    b, f, t = e1.shape[0], w.shape[0], w.shape[2]
    s = torch.matmul(torch.matmul(e1.permute(0, 2, 1), w.reshape(f, -1)).view(b, f, t).permute(0, 2, 1), e2)
    s = torch.relu(s + torch.matmul(p["tensor_network.weight_matrix_block"], torch.cat((e1, e2), dim=1)) +
                   p["tensor_network.bias"])
    s = torch.relu(Fn.linear(s.permute(0, 2, 1), p["fully_connected_first.weight"], p["fully_connected_first.bias"]))
    return torch.sigmoid(Fn.linear(s, p["scoring_layer.weight"], p["scoring_layer.bias"])).reshape(-1)


def train_step_loss(p, feats, target, idx_lists, eps=1e-5):
    """process_batch's forward: feats [2b, 3+L, N] for the graphs [A; B], target [b], the six kNN lists of [A; B].
    Two conv passes, as the reference: features_1 = [A; B], features_2 = [B; A].
    -> (mean BCE, predictions [2b], [stats of pass 1, stats of pass 2])."""
    b = feats.shape[0] // 2
    swap = lambda t: torch.cat((t[b:], t[:b]), dim=0)   # noqa: E731
    emb1, st1 = conv_pass(p, feats, idx_lists, eps)
    emb2, st2 = conv_pass(p, swap(feats), [swap(i) for i in idx_lists], eps)
    pred = forward_pair(p, emb1, emb2, None, None)
    tgt = torch.cat((target, target)).to(pred.dtype)
    return Fn.binary_cross_entropy(pred, tgt), pred, [st1, st2]


def running_after(buffers, stats_list, momentum=0.1):
    """BatchNorm's running-stat updates, one per conv pass: {name.1.running_mean / _var / num_batches_tracked}."""
    out = {k: v.clone() for k, v in buffers.items()}
    for stats in stats_list:
        for name, (m, v, count) in stats.items():
            rm, rv = name + ".1.running_mean", name + ".1.running_var"
            out[rm] = (1 - momentum) * out[rm] + momentum * m.to(out[rm].dtype)
            out[rv] = (1 - momentum) * out[rv] + momentum * (v * count / (count - 1)).to(out[rv].dtype)
            out[name + ".1.num_batches_tracked"] = out[name + ".1.num_batches_tracked"] + 1
    return out
