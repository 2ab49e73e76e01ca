"""Float64 reference of the pair-coupled tail - TenorNetworkModule.forward + fully_connected_first / ReLU + scoring_layer /
sigmoid (layers_batch.py:70-83, sg_net.py:131-136) - for any architecture (F, T, B read off the tensors), and the range
quantities the HIP tails' prep kernels reduce to choose their datapath.  TEST INFRASTRUCTURE: used by tests/, never by
the product.

Range quantities (sgpr_score.hip ntn_prep_body / ap_mode, sgpr_wide.hip wide_tail_prep_kernel / tail_in_range):
  am = max over row graphs r, neurons t, columns j of |A'_r[t][j]|,  A'_r[t][j] = sum_i e1_r[i] W[i][j][t] + Wb[t][F + j]
  um = max over r, t of |u_r[t]|,                                     u_r[t] = Wb[t][:F] . e1_r + bias[t]
  em = max over column graphs c, j of |e2_c[j]|
  l1 = max over r, t of sum_j |A'_r[t][j]|
A launch forms f16 planes only if am, em and um + K am em (K = 32 on the tuned tail, TFP = 64 on the any-shape one) stay
below 60000; on the tuned tail um + l1 em < 1024 picks the form whose low plane's ReLU rides on its conversion.
The head's fold is fold[o][t] = fc2_w[o] fc1_w[o][t]."""
import numpy as np

F16_SAFE = 60000.0
MODE2_BOUND = 1024.0
TUNED_K = 32        # the tuned tail's bound: |H| <= um + 32 am em
ANY_SHAPE_K = 64    # the any-shape tail's (sgpr_wide.hip TFP)


def _d(t):
    if hasattr(t, "detach"):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def tail_weights(sd):
    """The tail's tensors of a state dict (with or without the DataParallel `module.` prefix) in float64."""
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    return dict(w=_d(sd["tensor_network.weight_matrix"]),                       # [F, F, T]
                wb=_d(sd["tensor_network.weight_matrix_block"]),                # [T, 2F]
                bias=_d(sd["tensor_network.bias"]).reshape(-1),                 # [T]
                fc1_w=_d(sd["fully_connected_first.weight"]),                   # [B, T]
                fc1_b=_d(sd["fully_connected_first.bias"]).reshape(-1),         # [B]
                fc2_w=_d(sd["scoring_layer.weight"]).reshape(-1),               # [B]
                fc2_b=float(_d(sd["scoring_layer.bias"]).reshape(-1)[0]))


def fold(sd):
    """fold[o][t] = fc2_w[o] fc1_w[o][t] in float64 [B, T]."""
    p = tail_weights(sd)
    return p["fc2_w"][:, None] * p["fc1_w"]


def row_terms(p, rows):
    """(A' [R, T, F], u [R, T]) of the row graphs."""
    e1 = _d(rows)
    f = p["w"].shape[0]
    a = np.einsum("ri,ijt->rtj", e1, p["w"]) + p["wb"][None, :, f:]
    u = e1 @ p["wb"][:, :f].T + p["bias"]
    return a, u


def gates(sd, rows, cols):
    """{am, um, em, l1} of a launch on rows x cols (float64 of the fp32 inputs)."""
    p = tail_weights(sd)
    a, u = row_terms(p, rows)
    e2 = _d(cols)
    return dict(am=float(np.abs(a).max()) if a.size else 0.0, um=float(np.abs(u).max()) if u.size else 0.0,
                em=float(np.abs(e2).max()) if e2.size else 0.0,
                l1=float(np.abs(a).sum(axis=2).max()) if a.size else 0.0)


def bound(g, k=TUNED_K):
    """um + k am em: the tails' bound on |H|."""
    return g["um"] + k * g["am"] * g["em"]


def tail(sd, rows, cols):
    """Scores of every (row, column) pair in float64 -> dict:
         score [R, M], z [R, M] (the logit), h [R, M, T] (the tensor network's output),
         zmag [R, M] = sum_o |fc2_w[o]| (|fc1_b[o]| + sum_t |fc1_w[o][t]| hmag[t]),  hmag[t] = |u[t]| + sum_j |A'[t][j] e2[j]|:
                       the size of every term the tail sums (its conditioning: arithmetic that rounds each term relatively
                       by eps is off by O(eps zmag) in z)
       plus the range quantities of gates()."""
    p = tail_weights(sd)
    a, u = row_terms(p, rows)
    e2 = _d(cols)
    h = np.maximum(np.einsum("rtj,cj->rct", a, e2) + u[:, None, :], 0.0)
    hmag = np.einsum("rtj,cj->rct", np.abs(a), np.abs(e2)) + np.abs(u)[:, None, :]
    g = np.maximum(h @ p["fc1_w"].T + p["fc1_b"], 0.0)
    z = g @ p["fc2_w"] + p["fc2_b"]
    zmag = (np.abs(p["fc1_b"]) + hmag @ np.abs(p["fc1_w"]).T) @ np.abs(p["fc2_w"])
    out = dict(score=0.5 + 0.5 * np.tanh(0.5 * z), z=z, h=h, zmag=zmag)          # (the logistic without overflow)
    out.update(gates(sd, rows, cols))
    return out


# ------------------------------------------------------------------ checkpoint variants at the edges of the head's f16 range
NTN_KEYS = ("tensor_network.weight_matrix", "tensor_network.weight_matrix_block", "tensor_network.bias")
FC1 = "fully_connected_first.weight"


def _copy(sd):
    return {k: v.clone() for k, v in sd.items()}


def _key(sd, name):
    return [k for k in sd if k == name or k.endswith("." + name)][0]


def reparametrised(sd, c):
    """NTN W, Wb and bias times c, fc1_w divided by c: by ReLU homogeneity the same function; with c a power of two the
    fp32 tensors hold it exactly (H scales by c, the head's fold by 1 / c)."""
    out = _copy(sd)
    for name in NTN_KEYS:
        out[_key(out, name)] *= c
    out[_key(out, FC1)] /= c
    return out


def _pre_activations(sd, rows, cols):
    p = tail_weights(sd)
    a, u = row_terms(p, rows)
    return np.einsum("rtj,cj->rct", a, _d(cols)) + u[:, None, :]           # [R, M, T], before the ReLU


def dead_neuron_with_huge_fold(sd, inputs, magnitude=1e5):
    """Neuron t's bias set so that its pre-activation is below -1 on every pair of every (rows, cols) in `inputs`, then
    fc1_w[o][t] such that |fold[o][t]| = magnitude (o: the largest |fc2_w|): the float64 contribution is exactly 0."""
    out = _copy(sd)
    pre = np.concatenate([_pre_activations(sd, r, c).reshape(-1, tail_weights(sd)["bias"].size) for r, c in inputs])
    t = int(np.argmin((pre > 0).mean(axis=0)))                 # the least live neuron: the smallest bias shift
    kb = _key(out, "tensor_network.bias")
    shift = float(pre[:, t].max()) + 1.0
    out[kb].view(-1)[t] -= shift
    p = tail_weights(out)
    o = int(np.argmax(np.abs(p["fc2_w"])))
    out[_key(out, FC1)][o, t] = magnitude / p["fc2_w"][o]
    return out, t, o


def live_cancellation(sd, inputs, magnitude=1e5):
    """Neuron t (the most live one) copied into neuron t' (W[:, :, t], Wb[t], bias[t]), then fc1_w[o][t] += D and
    fc1_w[o][t'] -= D with |fc2_w[o] D| ~ magnitude (D a power of two, |fc2_w[o] D| in [magnitude / sqrt 2, magnitude sqrt 2]):
    H[t] = H[t'] is live and the two D terms cancel exactly in float64 (of the stored fp32 weights)."""
    out = _copy(sd)
    pre = np.concatenate([_pre_activations(sd, r, c).reshape(-1, tail_weights(sd)["bias"].size) for r, c in inputs])
    live = (pre > 0).mean(axis=0)
    t = int(np.argmax(live))
    t2 = int(np.argmin(live)) if int(np.argmin(live)) != t else (t + 1) % live.size
    kw, kwb, kbias = (_key(out, n) for n in NTN_KEYS)
    out[kw][:, :, t2] = out[kw][:, :, t]
    out[kwb][t2] = out[kwb][t]
    out[kbias].view(-1)[t2] = out[kbias].view(-1)[t]
    p = tail_weights(out)
    o = int(np.argmax(np.abs(p["fc2_w"])))
    d = float(2.0 ** np.round(np.log2(magnitude / abs(p["fc2_w"][o]))))
    w1 = out[_key(out, FC1)]
    w1[o, t] += d
    w1[o, t2] -= d
    return out, t, t2, o


def scale_to(sd, rows, cols, quantity, target, k=TUNED_K):
    """The input scale s (rows and columns both times s) at which a range quantity of the launch on (s rows) x (s cols)
    equals `target`: quantity in am, em, bound (um + k am em), mode2 (um + l1 em).  Bisection on log s (every quantity
    grows with s)."""
    def q(s):
        g = gates(sd, rows * np.float32(s), cols * np.float32(s))
        return dict(am=g["am"], em=g["em"], bound=bound(g, k), mode2=g["um"] + g["l1"] * g["em"])[quantity]
    lo, hi = 1e-6, 1e8
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        lo, hi = (mid, hi) if q(mid) < target else (lo, mid)
    return float(np.sqrt(lo * hi))
