"""Training: the reference's SGTrainer.fit / process_batch / score / augment_data (sg_net.py:208-422, utils.py:86-178)
over an `SG` module's own parameters.

The hot path is the EdgeConv block in train mode (edge features -> Conv2d 1x1 -> BatchNorm2d with batch statistics ->
LeakyReLU -> max over k).  `EdgeConvBN` runs it through sgpr_edgeconv_train_forward / _backward (csrc/sgpr_train.hip)
without the [B, 2C, N, k] edge tensor: the conv splits into two per-node products P = Wa x and Q = (Wb - Wa) x that
torch forms (and differentiates), and the kernels do the gather, the batch statistics, the selection of the max edge
and the backward through all of it.  conv_end (Conv1d + BatchNorm1d), attention, the tensor network, the head and the
BCE loss are small dense work in torch ops.  SG's inference engine is untouched: `SGFitter.score` runs on it.

`SGFitter(in_batch="all" | "balanced")` trains on every pose-labelled ordered pair among the 2 * batch graphs of a step
instead of the 2 * batch listed ones: `pair_classes` labels the G x G square on the host and `PairsTail` (tensor network
+ head + weighted BCE over the square, csrc/sgpr_train_pairs.hip) replaces the torch tail, forward and backward.

The reference feeds every pair twice (features_1 = [a, b], features_2 = [b, a]: sg_net.py:369-376), and both conv
passes see the same multiset of graphs, so the same batch statistics.  Here the 2 * batch distinct graphs are embedded
once, the pairs are the concatenations (pA, pB) and (pB, pA), and each BatchNorm running-stat update is applied twice,
which is what the reference's two calls do.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as Fn

from . import engine as _engine
from . import metrics
from .sg_net import SG, pack_graph
from .utils import load_paires, read_graph

NUM_LABELS = 12
LRELU_SLOPE = 0.2
NEG_DISTANCE = 20.0       # sg_net.py:302-309: a pair at >= 20 m is a negative


# ---------------------------------------------------------------------------------------------------- the fused op
def ctypes_stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _checked(lib, rc):
    if rc != _engine.SGPR_OK:
        raise _engine.SgprError(rc, lib.sgpr_last_error().decode())


class EdgeConvBN(torch.autograd.Function):
    """y [B,F,N] = max_k LeakyReLU(BN_train(P[b,f,idx[b,i,k]] + Q[b,f,i])) and the batch mean / biased variance [F].

    P, Q [B,F,N] f32 on the GPU, idx [B,N,k] int64 (sgpr_knn's lists), gamma / beta [F].  Differentiable in P, Q, gamma
    and beta; mean and var are returned for the running-stat update and carry no gradient."""

    @staticmethod
    def forward(ctx, P, Q, idx, gamma, beta, eps=1e-5):
        lib = _engine.load_library()
        if not P.is_cuda:
            raise RuntimeError("EdgeConvBN runs on the MI355X only (there is no CPU fallback)")
        P, Q = P.detach().float().contiguous(), Q.detach().float().contiguous()
        idx = idx.to(device=P.device, dtype=torch.int64).contiguous()
        gamma = gamma.detach().float().contiguous()
        beta = beta.detach().float().contiguous()
        b, f, n = P.shape
        k = idx.shape[2]
        if Q.shape != P.shape or tuple(idx.shape[:2]) != (b, n) or gamma.numel() != f or beta.numel() != f:
            raise ValueError("EdgeConvBN: P, Q [B,F,N], idx [B,N,k], gamma / beta [F]")
        dev = P.device
        y = torch.empty_like(P)
        sel = torch.empty(b, f, n, dtype=torch.uint8, device=dev)
        s1 = torch.empty_like(P)
        mean = torch.empty(f, dtype=torch.float32, device=dev)
        var = torch.empty(f, dtype=torch.float32, device=dev)
        ws_bytes = int(lib.sgpr_edgeconv_train_workspace_bytes(b, f))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        p = _engine._ptr
        with torch.cuda.device(dev):
            _checked(lib, lib.sgpr_edgeconv_train_forward(p(P), p(Q), p(idx), p(gamma), p(beta), b, f, n, k, float(eps),
                                                          p(y), p(sel), p(s1), p(mean), p(var), p(ws), ws_bytes,
                                                          ctypes_stream(P)))
        ctx.save_for_backward(P, Q, idx, sel, s1, mean, var, gamma, beta)
        ctx.eps = float(eps)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        lib = _engine.load_library()
        P, Q, idx, sel, s1, mean, var, gamma, beta = ctx.saved_tensors
        b, f, n = P.shape
        k = idx.shape[2]
        dy = dy.float().contiguous()
        dP, dQ = torch.empty_like(P), torch.empty_like(P)
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(beta)
        ws_bytes = int(lib.sgpr_edgeconv_train_workspace_bytes(b, f))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=P.device)
        p = _engine._ptr
        with torch.cuda.device(P.device):
            _checked(lib, lib.sgpr_edgeconv_train_backward(p(dy), p(P), p(Q), p(idx), p(sel), p(s1), p(mean), p(var),
                                                           p(gamma), p(beta), b, f, n, k, ctx.eps, p(dP), p(dQ),
                                                           p(dgamma), p(dbeta), p(ws), ws_bytes, ctypes_stream(P)))
        return dP, dQ, None, dgamma, dbeta, None


def edgeconv_bn(P, Q, idx, gamma, beta, eps=1e-5):
    """Functional form of EdgeConvBN -> (y, mean, biased var)."""
    return EdgeConvBN.apply(P, Q, idx, gamma, beta, eps)


class PairsTail(torch.autograd.Function):
    """Tensor network + head + weighted BCE over every ordered pair of rep [G,F] (sgpr_pairs_train_forward / _backward,
    csrc/sgpr_train_pairs.hip) -> (loss, pred [G,G], wsum).  cls [G,G] uint8: 0 = negative (weight w_neg), 1 = positive
    (w_pos), anything else = not in the loss.  W [F,F,T], V [T,2F], b [T], fc1_w [H,T], fc1_b [H], fc2_w [H], fc2_b [1].
    Differentiable in rep and the seven parameter tensors; pred and wsum carry no gradient."""

    @staticmethod
    def forward(ctx, rep, cls, W, V, b, fc1_w, fc1_b, fc2_w, fc2_b, w_neg=1.0, w_pos=1.0):
        lib = _engine.load_library()
        if not rep.is_cuda:
            raise RuntimeError("PairsTail runs on the MI355X only (there is no CPU fallback)")
        dev = rep.device
        shapes = (rep.shape, W.shape, V.shape, b.shape, fc1_w.shape, fc1_b.shape, fc2_w.shape, fc2_b.shape)
        rep, W, V, b, fc1_w, fc1_b, fc2_w, fc2_b = (t.detach().to(device=dev, dtype=torch.float32).contiguous()
                                                    for t in (rep, W, V, b, fc1_w, fc1_b, fc2_w, fc2_b))
        if rep.dim() != 2 or W.dim() != 3:
            raise ValueError("PairsTail: rep [G,F], W [F,F,T]")
        g, f = rep.shape
        t, h = W.shape[2], fc1_w.shape[0]
        cls = cls.to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(W.shape) != (f, f, t) or V.numel() != 2 * f * t or b.numel() != t or tuple(fc1_w.shape) != (h, t) or \
                fc1_b.numel() != h or fc2_w.numel() != h or fc2_b.numel() != 1 or tuple(cls.shape) != (g, g):
            raise ValueError("PairsTail: rep [G,F], cls [G,G], W [F,F,T], V [T,2F], b [T], fc1_w [H,T], fc1_b [H], "
                             "fc2_w [H], fc2_b [1]")
        pred = torch.empty(g, g, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        wsum = torch.empty((), dtype=torch.float32, device=dev)
        ws_bytes = int(lib.sgpr_pairs_train_workspace_bytes(g, f, t, h))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        p = _engine._ptr
        with torch.cuda.device(dev):
            _checked(lib, lib.sgpr_pairs_train_forward(p(rep), p(W), p(V), p(b), p(fc1_w), p(fc1_b), p(fc2_w), p(fc2_b),
                                                       p(cls), float(w_neg), float(w_pos), g, f, t, h, p(pred), p(loss),
                                                       p(wsum), p(ws), ws_bytes, ctypes_stream(rep)))
        ctx.save_for_backward(rep, cls, W, V, b, fc1_w, fc1_b, fc2_w, fc2_b, pred, wsum)
        ctx.weights = (float(w_neg), float(w_pos))
        ctx.shapes = shapes
        ctx.mark_non_differentiable(pred, wsum)
        return loss, pred, wsum

    @staticmethod
    def backward(ctx, dloss, _dpred, _dwsum):
        lib = _engine.load_library()
        rep, cls, W, V, b, fc1_w, fc1_b, fc2_w, fc2_b, pred, wsum = ctx.saved_tensors
        g, f = rep.shape
        t, h = W.shape[2], fc1_w.shape[0]
        dloss = dloss.detach().to(device=rep.device, dtype=torch.float32).reshape(1).contiguous()
        grads = [torch.empty_like(x) for x in (rep, W, V, b, fc1_w, fc1_b, fc2_w, fc2_b)]
        ws_bytes = int(lib.sgpr_pairs_train_workspace_bytes(g, f, t, h))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=rep.device)
        p = _engine._ptr
        with torch.cuda.device(rep.device):
            _checked(lib, lib.sgpr_pairs_train_backward(p(dloss), p(wsum), p(pred), p(rep), p(W), p(V), p(b), p(fc1_w),
                                                        p(fc1_b), p(fc2_w), p(fc2_b), p(cls), ctx.weights[0],
                                                        ctx.weights[1], g, f, t, h, *[p(x) for x in grads], p(ws),
                                                        ws_bytes, ctypes_stream(rep)))
        grads = [x.view(s) for x, s in zip(grads, ctx.shapes)]
        return (grads[0], None) + tuple(grads[1:]) + (None, None)


def pairs_tail(rep, cls, tensor_network, fully_connected_first, scoring_layer, w_neg=1.0, w_pos=1.0):
    """The training tail over all G x G ordered pairs of rep [G,F] (PairsTail) with the modules' own parameters
    -> (loss, pred [G,G], wsum)."""
    return PairsTail.apply(rep, cls, tensor_network.weight_matrix, tensor_network.weight_matrix_block,
                           tensor_network.bias, fully_connected_first.weight, fully_connected_first.bias,
                           scoring_layer.weight, scoring_layer.bias, w_neg, w_pos)


# ---------------------------------------------------------------------------------------------------- model forward
def _update_running(bn, mean, var, count, times):
    """BatchNorm's running-stat update (momentum, unbiased variance), applied `times` times, in place (bumps _version:
    SG.engine() sees the new statistics)."""
    with torch.no_grad():
        m = bn.momentum
        unbiased = var * (count / max(count - 1, 1))
        for _ in range(times):
            bn.running_mean.mul_(1.0 - m).add_(mean.to(bn.running_mean.dtype), alpha=m)
            bn.running_var.mul_(1.0 - m).add_(unbiased.to(bn.running_var.dtype), alpha=m)
        bn.num_batches_tracked.add_(times)


def edgeconv_block(x, block, k, updates=2, idx=None):
    """One `nn.Sequential(Conv2d 1x1, BatchNorm2d, LeakyReLU)` EdgeConv block in train mode on x [B,C,N]
    -> (y [B,F,N], idx [B,N,k]).  idx: the kNN lists of x (sgpr_knn on x itself, like get_graph_feature, when None)."""
    conv, bn = block[0], block[1]
    b, c, n = x.shape
    w = conv.weight.view(conv.weight.shape[0], 2 * c)
    wa, wb = w[:, :c], w[:, c:]
    if idx is None:
        idx = _engine.knn(x.detach(), k)
    P = torch.matmul(wa, x)
    Q = torch.matmul(wb - wa, x)
    y, mean, var = EdgeConvBN.apply(P, Q, idx, bn.weight, bn.bias, bn.eps)
    if updates:
        _update_running(bn, mean, var, b * n * int(idx.shape[2]), updates)
    return y, idx


def dense_features(centers, labels, num_labels=NUM_LABELS):
    """Packed graphs (centers [G,N,3], labels [G,N], -1 = pad) -> features [G, 3 + L, N] (sg_net.py:274-299)."""
    lab = labels.long()
    onehot = Fn.one_hot(lab.clamp(min=0), num_labels).to(centers.dtype) * (lab >= 0).unsqueeze(-1).to(centers.dtype)
    return torch.cat((centers, onehot), dim=2).permute(0, 2, 1).contiguous()


def embed_train(model, feats, updates=2, idx_lists=None):
    """SG.dgcnn_conv_pass (sg_net.py:79-110) in train mode: feats [G, 3 + L, N] -> (node embeddings [G, N, F3], the six
    kNN lists in the order s1, s2, s3, f1, f2, f3)."""
    k = int(model.args.K)
    lists = []

    def branch(x, blocks, first):
        for j, blk in enumerate(blocks):
            x, idx = edgeconv_block(x, blk, k, updates, None if idx_lists is None else idx_lists[first + j])
            lists.append(idx)
        return x

    xyz = branch(feats[:, :3, :], (model.dgcnn_s_conv1, model.dgcnn_s_conv2, model.dgcnn_s_conv3), 0)
    sem = branch(feats[:, 3:, :], (model.dgcnn_f_conv1, model.dgcnn_f_conv2, model.dgcnn_f_conv3), 3)
    x = torch.cat((xyz, sem), dim=1)
    conv, bn = model.dgcnn_conv_end[0], model.dgcnn_conv_end[1]
    x = torch.matmul(conv.weight.view(conv.weight.shape[0], -1), x)
    if updates:
        with torch.no_grad():
            _update_running(bn, x.mean(dim=(0, 2)), x.var(dim=(0, 2), unbiased=False), x.shape[0] * x.shape[2], updates)
    x = Fn.batch_norm(x, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)   # batch statistics
    x = Fn.leaky_relu(x, LRELU_SLOPE)
    return x.permute(0, 2, 1), lists


def attention(module, emb):
    """AttentionModule.forward (layers_batch.py:28-39) in torch ops: emb [G,N,F] -> (rep [G,F,1], scores [G,N,1])."""
    g = emb.shape[0]
    ctx = torch.tanh(torch.mean(torch.matmul(emb, module.weight_matrix), dim=1))
    scores = torch.sigmoid(torch.matmul(emb, ctx.view(g, -1, 1)))
    return torch.matmul(emb.permute(0, 2, 1), scores), scores


def tensor_network(module, e1, e2):
    """TenorNetworkModule.forward (layers_batch.py:70-83) in torch ops: e1, e2 [B,F,1] -> [B,T,1]."""
    b, f = e1.shape[0], module.weight_matrix.shape[0]
    t = module.weight_matrix.shape[2]
    s = torch.matmul(e1.permute(0, 2, 1), module.weight_matrix.view(f, -1)).view(b, f, t)
    s = torch.matmul(s.permute(0, 2, 1), e2)
    block = torch.matmul(module.weight_matrix_block, torch.cat((e1, e2), dim=1))
    return Fn.relu(s + block + module.bias)


def head(model, scores):
    """sg_net.py:128-137: [B,T,1] -> score [B]."""
    s = Fn.relu(model.fully_connected_first(scores.permute(0, 2, 1)))
    return torch.sigmoid(model.scoring_layer(s)).reshape(-1)


def train_loss(model, feats, target, updates=2, idx_lists=None):
    """One train-mode forward of process_batch (sg_net.py:358-383) on 2b graphs ordered [A_0..A_b-1, B_0..B_b-1]:
    the pairs (A_p, B_p) and (B_p, A_p) with target [b] each -> (mean BCE, predictions [2b], the six kNN lists)."""
    b = feats.shape[0] // 2
    emb, lists = embed_train(model, feats, updates, idx_lists)
    rep, _ = attention(model.attention, emb)
    e1 = torch.cat((rep[:b], rep[b:]), dim=0)
    e2 = torch.cat((rep[b:], rep[:b]), dim=0)
    pred = head(model, tensor_network(model.tensor_network, e1, e2))
    tgt = torch.cat((target, target)).to(pred.dtype)
    return Fn.binary_cross_entropy(pred, tgt), pred, lists


def train_loss_in_batch(model, feats, cls, w_neg=1.0, w_pos=1.0, updates=2, idx_lists=None):
    """One train-mode forward on G graphs that trains on every labelled ordered pair among them: embed_train and
    attention as train_loss, then pairs_tail on the pooled vectors -> (weighted mean BCE, predictions [G,G], the six
    kNN lists).  cls [G,G] uint8 as pair_classes gives it."""
    emb, lists = embed_train(model, feats, updates, idx_lists)
    rep, _ = attention(model.attention, emb)
    loss, pred, _ = pairs_tail(rep[:, :, 0], cls, model.tensor_network, model.fully_connected_first,
                               model.scoring_layer, w_neg, w_pos)
    return loss, pred, lists


# ---------------------------------------------------------------------------------------------------- augmentation
def _rot_z(angle):
    c, s = torch.cos(angle), torch.sin(angle)
    o, z = torch.ones_like(angle), torch.zeros_like(angle)
    return torch.stack((c, -s, z, s, c, z, z, z, o), dim=1).view(-1, 3, 3)


def _rot_y(angle):
    c, s = torch.cos(angle), torch.sin(angle)
    o, z = torch.ones_like(angle), torch.zeros_like(angle)
    return torch.stack((c, z, s, z, o, z, -s, z, c), dim=1).view(-1, 3, 3)


def _rot_x(angle):
    c, s = torch.cos(angle), torch.sin(angle)
    o, z = torch.ones_like(angle), torch.zeros_like(angle)
    return torch.stack((o, z, z, z, c, -s, z, s, c), dim=1).view(-1, 3, 3)


def augment(centers, generator, shared_flip=False):
    """transfer_to_torch's training branch (sg_net.py:286-292) + augment_data (sg_net.py:226-233, utils.py:86-178) on
    the device, for 2b packed graphs ordered [A_0..A_b-1, B_0..B_b-1] (centers [2b, N, 3]) -> new f32 tensor.

    In the reference's order and with its distributions: one x-flip with p = 0.5 shared by both graphs of a pair; then
    per graph a rotation about z by U(0, 2 pi), a jitter N(0, 0.01) clipped to +-0.05 per coordinate, a scale U(0.8,
    1.25), a small rotation R = Rz Ry Rx with angles N(0, 0.015) clipped to +-0.045, and a shift U(-0.3, 0.3) per axis.
    Points are row vectors (p' = p R), as np.dot(shape_pc, R).  Padded slots are transformed too, as in the reference.
    The draws come from `generator` (a torch.Generator on the centres' device), not from the global RNGs.
    shared_flip: the x-flip is ONE draw for the whole batch (a mirrored scan is not the place its unmirrored neighbour
    shows, and in-batch pairs join graphs of different listed pairs); every other draw keeps its distribution and order."""
    g, n, _ = centers.shape
    b = g // 2
    dev = centers.device
    x = centers.to(torch.float64)

    def rand(*shape):
        return torch.rand(*shape, generator=generator, device=dev, dtype=torch.float64)

    def randn(*shape):
        return torch.randn(*shape, generator=generator, device=dev, dtype=torch.float64)

    if shared_flip:
        flip = (rand(1) > 0.5).expand(g)
    else:
        flip = rand(b) > 0.5
        flip = torch.cat((flip, flip))
    x = torch.cat((torch.where(flip.view(g, 1, 1), -x[..., :1], x[..., :1]), x[..., 1:]), dim=2)
    x = torch.bmm(x, _rot_z(rand(g) * (2.0 * math.pi))).to(torch.float32).to(torch.float64)   # utils.py: f32 result
    x = x + torch.clamp(0.01 * randn(g, n, 3), -0.05, 0.05)
    x = x * (0.8 + 0.45 * rand(g)).view(g, 1, 1)
    ang = torch.clamp(0.015 * randn(g, 3), -0.045, 0.045)
    r = torch.bmm(_rot_z(ang[:, 2]), torch.bmm(_rot_y(ang[:, 1]), _rot_x(ang[:, 0])))
    x = torch.bmm(x, r).to(torch.float32).to(torch.float64)
    x = x + (rand(g, 1, 3) * 0.6 - 0.3)
    return x.to(torch.float32)


# ---------------------------------------------------------------------------------------------------- data
def target_of(distance, p_thresh):
    """sg_net.py:302-309: 1 at <= p_thresh, 0 at >= 20 m; anything between ends the run, as in the reference."""
    if distance <= p_thresh:
        return 1.0
    if distance >= NEG_DISTANCE:
        return 0.0
    print("distance error: ", distance)
    sys.exit(-1)


def pair_classes(xz, graph_ids, sequence=None, p_thresh=3.0, d_neg=NEG_DISTANCE):
    """The class of every ordered pair of a batch, by target_of's rule: xz [n,2] planar poses (float64), graph_ids [G]
    the batch's slots (indices into xz, repeats allowed) -> uint8 [G,G]: 1 at distance <= p_thresh, 0 at >= d_neg, 2
    (not in the loss) in between, on the diagonal and between graphs of different `sequence` ids (their poses are in
    different frames).  PairSet._targets' arithmetic: sqrt(dx*dx + dz*dz) in float64."""
    xz = np.asarray(xz, dtype=np.float64)
    ids = np.asarray(graph_ids, dtype=np.int64).reshape(-1)
    p = xz[ids]
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(2))
    cls = np.full(d.shape, 2, dtype=np.uint8)
    cls[d <= p_thresh] = 1
    cls[d >= d_neg] = 0
    if sequence is not None:
        sq = np.asarray(sequence, dtype=np.int64).reshape(-1)[ids]
        cls[sq[:, None] != sq[None, :]] = 2
    np.fill_diagonal(cls, 2)
    return cls


def _planar(poses):
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 2 or poses.shape[1] not in (2, 12):
        raise ValueError("poses must be [G, 12] (KITTI 3x4; x = [3], z = [11]) or [G, 2] planar (x, z)")
    return poses[:, [3, 11]] if poses.shape[1] == 12 else poses


class PairSet(object):
    """Packed graphs (centers f32 [G,N,3], labels i32 [G,N], -1 = pad), their poses and the train / eval pair index
    arrays [P,2] into them: what SGFitter trains on.  Targets follow the reference's rule (target_of).
    sequence: one id per graph (int [G]): poses of different sequences are in different frames, so hard pairs are mined
    within one sequence only; None = one sequence."""

    def __init__(self, centers, labels, poses, train_pairs, eval_pairs, p_thresh=3.0, sequence=None):
        self.centers = np.ascontiguousarray(centers, dtype=np.float32)
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        xz = _planar(poses)
        if self.centers.ndim != 3 or self.centers.shape[2] != 3 or self.labels.shape != self.centers.shape[:2] or \
                len(xz) != len(self.labels):
            raise ValueError("centers [G,N,3], labels [G,N] and poses [G,.] must describe the same G graphs")
        self.xz = np.ascontiguousarray(xz, dtype=np.float64)
        self.p_thresh = float(p_thresh)
        self.sequence = None if sequence is None else np.asarray(sequence, dtype=np.int64).reshape(-1)
        if self.sequence is not None and len(self.sequence) != len(self.labels):
            raise ValueError("sequence must hold one id per graph (%d), got %d" % (len(self.labels), len(self.sequence)))
        self.train_pairs = np.asarray(train_pairs, dtype=np.int64).reshape(-1, 2)
        self.eval_pairs = np.asarray(eval_pairs, dtype=np.int64).reshape(-1, 2)
        for pairs in (self.train_pairs, self.eval_pairs):
            if len(pairs) and (pairs.min() < 0 or pairs.max() >= len(self.labels)):
                raise ValueError("pair index outside [0, %d)" % len(self.labels))
        self.train_targets = self._targets(xz, self.train_pairs, p_thresh)
        self.eval_targets = self._targets(xz, self.eval_pairs, p_thresh)

    @staticmethod
    def _targets(xz, pairs, p_thresh):
        d = np.sqrt(((xz[pairs[:, 0]] - xz[pairs[:, 1]]) ** 2).sum(1)) if len(pairs) else np.zeros(0)
        return np.array([target_of(float(v), p_thresh) for v in d], dtype=np.float32)

    @classmethod
    def from_files(cls, args, number_of_labels=NUM_LABELS):
        """The reference's file layer (sg_net.py:182-199): <pair_list_dir>/<seq>.txt for train_sequences and
        eval_sequences (utils.load_paires), graph JSONs under graph_pairs_dir.  Every graph is read and packed once."""
        seq_id = {}

        def lists(seqs):
            out = []
            for sq in seqs:
                sid = seq_id.setdefault(str(sq), len(seq_id))
                out.extend((a, b, sid) for a, b in load_paires(os.path.join(args.pair_list_dir, str(sq) + ".txt"),
                                                              args.graph_pairs_dir))
            return out

        train, evl = lists(args.train_sequences), lists(args.eval_sequences)
        if not train or not evl:
            raise ValueError("no training or no evaluation pairs (train_sequences / eval_sequences / pair_list_dir)")
        slot, centers, labels, poses, sequence = {}, [], [], [], []

        def index(path, sid):
            if path not in slot:
                d = read_graph(path)
                c, l = pack_graph(d["centers"], d["nodes"], int(args.node_num), number_of_labels)
                slot[path] = len(centers)
                centers.append(c)
                labels.append(l)
                poses.append(d["pose"])
                sequence.append(sid)             # (a graph file lives in its sequence's list: the first one naming it)
            return slot[path]

        tp = [[index(a, s), index(b, s)] for a, b, s in train]
        ep = [[index(a, s), index(b, s)] for a, b, s in evl]
        return cls(np.stack(centers), np.stack(labels), np.asarray(poses, dtype=np.float64), tp, ep, args.p_thresh,
                   sequence=np.asarray(sequence, dtype=np.int64))


def mined_pairs(groups, base_pairs):
    """Mined lists -> new unordered training pairs (pure function).
    groups: [(members int [n], indices int [n, k]), ...] - row r of a mining call over the graphs `members` (rows = columns
    = one sequence) listed columns indices[r] (-1 = empty slot).  Every (members[r], members[c]) becomes the unordered pair
    (min, max); duplicates and the pairs already in base_pairs (in either order) are dropped.  -> int64 [P, 2], sorted."""
    out = []
    for members, idx in groups:
        members = np.asarray(members, dtype=np.int64)
        idx = np.asarray(idx, dtype=np.int64)
        r, c = np.nonzero(idx >= 0)
        a, b = members[r], members[idx[r, c]]
        out.append(np.stack((np.minimum(a, b), np.maximum(a, b)), axis=1))
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    if len(pairs) == 0:
        return np.zeros((0, 2), np.int64)
    pairs = np.unique(pairs, axis=0)
    base = np.asarray(base_pairs, dtype=np.int64).reshape(-1, 2)
    if len(base):
        key = lambda p: p[:, 0] * (1 << 32) + p[:, 1]                                        # noqa: E731
        known = key(np.stack((base.min(1), base.max(1)), axis=1))
        pairs = pairs[~np.isin(key(pairs), known)]
    return pairs


def batches_of(n, batch_size, rng):
    """create_batches (sg_net.py:208-223): a shuffled order of n pairs cut into lists of batch_size."""
    order = rng.permutation(n)
    return [order[i:i + batch_size] for i in range(0, n, batch_size)]


def checkpoint_state(model):
    """The model's 50 tensors under the DataParallel `module.` prefix the reference saves (sg_net.py:404-410)."""
    return OrderedDict(("module." + k, v.detach().cpu().clone()) for k, v in model.state_dict().items())


# ---------------------------------------------------------------------------------------------------- the fitter
class SGFitter(object):
    """The training half of SGTrainer (sg_net.py:141-422) on the HIP EdgeConv op.

    SGFitter(args, init=None, seed=0, data=None): data is a PairSet (the in-memory entry point); None reads the
    reference's pair lists and graph JSONs (PairSet.from_files).  init loads a checkpoint (with or without the
    `module.` prefix) for fine-tuning; the reference always starts from scratch.  seed fixes the initial weights, the
    batch order and the augmentation.  in_batch: "off" trains on the listed pairs (both orders), as the reference;
    "all" embeds the same 2b slots of every batch and trains on EVERY labelled ordered pair among them (pair_classes)
    with weight 1; "balanced" weighs the positives of a batch by n_neg / n_pos when both are present."""

    LOG_NAME = "train_log.jsonl"

    IN_BATCH = ("off", "all", "balanced")

    def __init__(self, args, init=None, seed=0, data=None, hard_negatives=0, hard_positives=0, mine_every=2,
                 in_batch="off"):
        self.args = args
        if in_batch not in self.IN_BATCH:
            raise ValueError("in_batch must be one of %s" % (self.IN_BATCH,))
        self.in_batch = in_batch
        self.last_step = None        # in-batch modes: {"pairs_in_loss", "positives", "negatives"} of the latest step
        self.hard_negatives, self.hard_positives = int(hard_negatives), int(hard_positives)
        self.mine_every = int(mine_every)
        for k in (self.hard_negatives, self.hard_positives):
            if k < 0 or k > 16:
                raise ValueError("hard_negatives / hard_positives must lie in 0..16 (the mining lists' length)")
        if self.mine_every < 1:
            raise ValueError("mine_every must be >= 1")
        self.seed = int(seed)
        self.number_of_labels = NUM_LABELS
        self.device = torch.device("cuda", int(getattr(args, "gpu", 0)))
        self.data = data if data is not None else PairSet.from_files(args, self.number_of_labels)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.model = SG(args, self.number_of_labels)
        if init:
            sd = torch.load(init, map_location="cpu") if isinstance(init, (str, os.PathLike)) else init
            self.model.load_state_dict(OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in sd.items()))
        self.model.to(self.device)
        self.model.train()
        self.centers = torch.from_numpy(self.data.centers).to(self.device)
        self.labels = torch.from_numpy(self.data.labels).to(self.device)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(self.seed)
        self.rng = np.random.default_rng(self.seed)
        self.augment = True
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=args.learning_rate, weight_decay=args.weight_decay)
        self.f1_max_best = 0.0
        self.last_mined = None       # the latest self.mine() of fit (pairs, targets, lists, seconds)

    # ---------------------------------------------------------------- one batch
    def batch(self, pairs, training=True):
        """Pairs [b, 2] of graph indices -> (features [2b, 3 + L, N] of the graphs [A..., B...], their packed centres
        and labels).  training: the reference's augmentation (when self.augment)."""
        g = torch.from_numpy(np.concatenate((pairs[:, 0], pairs[:, 1]))).to(self.device)
        centers, labels = self.centers[g], self.labels[g]
        if training and self.augment:
            centers = augment(centers, self.generator, shared_flip=self.in_batch != "off")
        return dense_features(centers, labels, self.number_of_labels), centers, labels

    def step(self, pair_ids, pairs=None, targets=None):
        """process_batch(training=True) (sg_net.py:358-387) on the train pairs pair_ids -> loss (float).
        pairs / targets: the epoch's pair list when it is not data.train_pairs (base + mined pairs)."""
        self.model.train()
        pairs_all = self.data.train_pairs if pairs is None else pairs
        targets_all = self.data.train_targets if targets is None else targets
        pairs = pairs_all[pair_ids]
        feats, _, _ = self.batch(pairs, True)
        self.optimizer.zero_grad(set_to_none=True)
        if self.in_batch != "off":
            cls = pair_classes(self.data.xz, np.concatenate((pairs[:, 0], pairs[:, 1])), self.data.sequence,
                               self.data.p_thresh)
            n_pos, n_neg = int((cls == 1).sum()), int((cls == 0).sum())
            w_pos = n_neg / n_pos if self.in_batch == "balanced" and n_pos and n_neg else 1.0
            self.last_step = {"pairs_in_loss": n_pos + n_neg, "positives": n_pos, "negatives": n_neg}
            loss, _, _ = train_loss_in_batch(self.model, feats, torch.from_numpy(cls).to(self.device), 1.0, w_pos)
            loss.backward()
            self.optimizer.step()
            return float(loss.item())
        target = torch.from_numpy(targets_all[pair_ids]).to(self.device)
        loss, _, _ = train_loss(self.model, feats, target)
        loss.backward()
        self.optimizer.step()
        return float(loss.item())

    # ---------------------------------------------------------------- evaluation on the inference engine
    def score(self, split="eval"):
        """score (sg_net.py:412-446): mean BCE per batch and F1-max over the evaluation pairs, both orders of every pair,
        on the inference engine (model.eval(); the engine is rebuilt from the current weights)."""
        if split not in ("eval", "test"):
            print("Check split: ", split)
            sys.exit(-1)
        self.model.eval()
        pairs, targets = self.data.eval_pairs, self.data.eval_targets
        bs = int(self.args.batch_size)
        preds, gts, losses = [], [], []
        with torch.no_grad():
            for i in range(0, len(pairs), bs):
                p = pairs[i:i + bs]
                b = len(p)
                _, centers, labels = self.batch(p, False)
                pooled, _, _ = self.model.embed(centers, labels)
                self.model.engine().check_status()
                s = torch.cat((self.model.score_pooled(pooled[:b], pooled[b:]),
                               self.model.score_pooled(pooled[b:], pooled[:b]))).float()
                t = torch.from_numpy(np.concatenate((targets[i:i + bs], targets[i:i + bs]))).to(s.device)
                losses.append(float(Fn.binary_cross_entropy(s.clamp(0.0, 1.0), t).item()))
                preds.append(s.cpu().numpy())
                gts.append(t.cpu().numpy())
        self.model.train()
        if not losses:
            return float("nan"), 0.0
        f1 = float(metrics.f1_max(np.concatenate(gts), np.concatenate(preds)))
        loss = float(np.mean(losses))
        print("\nModel " + split + " F1_max_score: " + str(f1) + ".")
        print("\nModel " + split + " loss: " + str(loss) + ".")
        return loss, f1

    # ---------------------------------------------------------------- hard-pair mining
    def mine(self):
        """The hardest pairs of the current weights (Engine.score_mine): the model in eval mode embeds, without
        augmentation, the graphs that appear in train_pairs on the inference engine; per sequence, every graph takes its
        hard_negatives highest-scoring graphs at >= 20 m and its hard_positives lowest-scoring graphs within p_thresh.
        No BatchNorm statistic moves and self.generator is not drawn from.
        -> {"pairs" int64 [P,2] (new unordered pairs, base pairs dropped), "targets" f32 [P], "lists": [(sequence id,
        members, positives, values, indices), ...], "seconds"}"""
        t0 = time.perf_counter()
        data = self.data
        used = np.unique(data.train_pairs)
        seq = data.sequence if data.sequence is not None else np.zeros(len(data.labels), np.int64)
        was_training = self.model.training
        self.model.eval()
        lists, groups = [], []
        try:
            with torch.no_grad():
                eng = self.model.engine()
                for sid in np.unique(seq[used]):
                    members = used[seq[used] == sid]
                    g = torch.from_numpy(members).to(self.device)
                    pooled, _, _ = self.model.embed(self.centers[g], self.labels[g])
                    eng.check_status()
                    for positives, k in ((False, self.hard_negatives), (True, self.hard_positives)):
                        if k == 0:
                            continue
                        v, i = eng.score_mine(pooled, pooled, data.xz[members], k=k, positives=positives,
                                              d_pos=data.p_thresh, d_neg=NEG_DISTANCE)
                        v, i = v.cpu().numpy(), i.cpu().numpy()
                        lists.append((int(sid), members, positives, v, i))
                        groups.append((members, i))
        finally:
            if was_training:
                self.model.train()
        pairs = mined_pairs(groups, data.train_pairs)
        targets = PairSet._targets(data.xz, pairs, data.p_thresh)
        return {"pairs": pairs, "targets": targets, "lists": lists, "seconds": time.perf_counter() - t0}

    def _mines(self, epoch):
        return (self.hard_negatives > 0 or self.hard_positives > 0) and epoch >= self.mine_every and \
            epoch % self.mine_every == 0

    # ---------------------------------------------------------------- the loop
    def _log(self, record):
        os.makedirs(self.args.logdir, exist_ok=True)
        with open(os.path.join(self.args.logdir, self.LOG_NAME), "a") as f:
            f.write(json.dumps(record) + "\n")

    def save(self, epoch, best=False):
        os.makedirs(self.args.logdir, exist_ok=True)
        path = os.path.join(self.args.logdir, "%d%s.pth" % (epoch, "_best" if best else ""))
        torch.save(checkpoint_state(self.model), path)
        return path

    def fit(self, epochs=None):
        """fit (sg_net.py:389-410): Adam(lr, weight_decay); every epoch one shuffled pass over the train pairs; every
        second epoch (0, 2, ...) score("eval"), <epoch>.pth, and <epoch>_best.pth when F1-max >= the best so far.
        Progress goes to <logdir>/train_log.jsonl, one JSON object per line.  With hard_negatives / hard_positives, every
        epoch e >= mine_every with e % mine_every == 0 first mines (self.mine) and trains on the base plus the mined
        pairs; the log records their count and the time mining took."""
        epochs = int(self.args.epochs if epochs is None else epochs)
        bs = int(self.args.batch_size)
        for epoch in range(epochs):
            seen, loss_sum = 0, 0.0
            pairs = targets = None
            if self._mines(epoch):
                mined = self.mine()
                self.last_mined = mined
                pairs = np.concatenate((self.data.train_pairs, mined["pairs"]))
                targets = np.concatenate((self.data.train_targets, mined["targets"]))
                self._log({"epoch": epoch, "mined_pairs": int(len(mined["pairs"])),
                           "mined_negatives": int((mined["targets"] == 0).sum()),
                           "mined_positives": int((mined["targets"] == 1).sum()), "mine_seconds": mined["seconds"]})
            n = len(self.data.train_pairs) if pairs is None else len(pairs)
            for ids in batches_of(n, bs, self.rng):
                loss = self.step(ids, pairs, targets)
                seen += len(ids)
                loss_sum += loss * len(ids)
                rec = {"epoch": epoch, "pairs": seen, "loss": loss, "loss_avg": loss_sum / seen}
                if self.in_batch != "off":
                    rec.update(self.last_step)
                self._log(rec)
            if epoch % 2 == 0:
                eval_loss, f1 = self.score("eval")
                rec = {"epoch": epoch, "eval_loss": eval_loss, "f1_max": f1, "checkpoint": self.save(epoch)}
                if self.f1_max_best <= f1:
                    self.f1_max_best = f1
                    rec["best"] = self.save(epoch, best=True)
                self._log(rec)
        return self


# ---------------------------------------------------------------------------------------------------- CLI
def parse_cli(argv=None):
    p = argparse.ArgumentParser(prog="python -m sg_pr_amd.main_sg",
                                description="Train SG_PR (main_sg.py): fit, then score on the evaluation pairs.")
    p.add_argument("config", nargs="?", default="./config/config.yml")
    p.add_argument("--epochs", type=int, default=None, help="override train.epochs of the config")
    p.add_argument("--init", default=None, help="checkpoint to fine-tune from (default: a fresh model)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--hard-negatives", type=int, default=0, metavar="K",
                   help="per graph and mining epoch, add its K highest-scoring pairs at >= 20 m (0..16; default 0: off)")
    p.add_argument("--hard-positives", type=int, default=0, metavar="K",
                   help="per graph and mining epoch, add its K lowest-scoring pairs within p_thresh (0..16; default 0)")
    p.add_argument("--mine-every", type=int, default=2, metavar="E",
                   help="mine at the start of every epoch e >= E with e %% E == 0 (default 2)")
    p.add_argument("--in-batch", choices=SGFitter.IN_BATCH, default="off",
                   help="train on every pose-labelled ordered pair among the graphs of a batch: all = weight 1, "
                        "balanced = positives weighted by n_neg / n_pos per batch (default off: the listed pairs)")
    return p.parse_args(argv)


def main(argv=None):
    from .parser_sg import sgpr_args
    from .utils import tab_printer
    cli = parse_cli(argv)
    args = sgpr_args()
    args.load(cli.config)
    if cli.epochs is not None:
        args.epochs = cli.epochs
    tab_printer(args)
    fitter = SGFitter(args, init=cli.init, seed=cli.seed, hard_negatives=cli.hard_negatives,
                      hard_positives=cli.hard_positives, mine_every=cli.mine_every, in_batch=cli.in_batch)
    fitter.fit()
    fitter.score()
    return fitter
