"""The any-shape kernels at every limit and dispatch boundary, against tests/any_shape_ref.py (float64, the library's tie
rule).  One table drives the embed sweep; tests/test_any_shape_ref_host.py imports it and asserts, on a CPU, that every
row keeps the cap on unsettled graphs the comparisons below rely on.  Needs a real MI355X: `pytest -m gpu`.

A model that is not exactly {12 labels, 64, 64, 32, 16, 16} takes one of four routes (include/sgpr.h, sgpr_dims):
  tuned    no larger in any of the six: the tuned kernels, the model zero-padded at sgpr_create (pooled width 32)
  wide64   any-shape handle, labels <= 32, filters <= 128 / 128 / 64, node_num <= 112, K = 10: two-plane matrix-core embed
  wide128  (sgpr_wide.hip); its <64,32> instance when every width padded to 32 is <= 64 / 64 / 32, else <128,64>
  plain    everything else: sgpr_generic.hip, working set in LDS up to 156 KB, else in a global scratch area
The all-pairs tail of an any-shape handle runs on the matrix cores when the embed's model limits hold and filters_3 <= 64,
tensor / bottleneck neurons <= 32; else on the plain kernel (instances of 16 / 32 / 64 tensor neurons).
What a test can OBSERVE of this through the ABI is asserted: any_shape / pooled width, whether debug bit 23 (plain fp32
only) changes the bits, whether the workspace grows per graph (global scratch) and what sgpr_embed_lds_bytes answers.  Which
of the two template instances of the two-plane embed runs is not observable; the table states it from wide_narrow's rule.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import any_shape_ref as ref64   # noqa: E402

SCORE_TOL = 1e-4        # the project's gates (tests/test_gpu_parity.py)
EMB_GATE = 1e-4         # * max(1, |ref|max)
POOLED_GATE = 2e-4      # * max(1, |ref|max)
ATT_GATE = 1e-4
ROUTE_GATE = 1e-4       # two-plane against plain, * scale
TAIL_ROUTE_GATE = 2e-5  # matrix-core tail against plain
LIST_GATE = 5e-5        # list kernels against the rectangle
PLAIN_BIT = 1 << 23

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAXM = (64, 256, 256, 128, 64, 64)
M13 = (13, 64, 64, 32, 16, 16)
LDS_SWITCH = 156 * 1024


def plain_lds_fit(dims, k):
    """largest node_num whose plain-kernel working set, 4 (N (3 cmax + f3 + 1 + K) + 64) bytes, stays within the 156 KB
    switch (sgpr_generic.hip).  The GPU test takes the same number from sgpr_embed_lds_bytes and asserts they agree."""
    labels, f1, f2, f3 = dims[:4]
    cmax = max(3, labels, f1, f2, f3)
    return (LDS_SWITCH // 4 - 64) // (3 * cmax + f3 + 1 + k)


# (real nodes, graph seed[, "spread"]) per graph of every row: the pairs that meet the cap at the measured tau - all
# padding, one real node, N real nodes, N - 1, then the fullest graphs that are settled (a full graph of more than ~65
# random nodes rarely is; where a row keeps one it runs and is held to everything but the numbers).  "spread" graphs put
# their real nodes at evenly spaced slots up to N - 1 (one_graph): they make the last row tiles and candidate blocks hold
# distinct nodes in a settled graph.  `python tests/any_shape_ref.py` prints every graph's smallest margin;
# tests/test_any_shape_ref_host.py::test_every_sweep_row_keeps_the_cap re-checks the cap.
FILLS = {
    "tuned-1x6-n24": [(0, 0), (1, 0), (24, 0), (23, 10), (19, 2), (14, 0), (9, 1), (4, 0)],
    "tuned-below-n64": [(0, 0), (1, 0), (64, 20), (63, 6), (51, 2), (38, 0), (25, 1), (12, 0)],
    "w64-m13-n10": [(0, 0), (1, 0), (10, 0), (9, 0), (8, 0), (6, 0), (4, 0), (2, 0)],
    "w64-l32f33t17-n16": [(0, 0), (1, 0), (16, 5), (15, 3), (12, 0), (9, 0), (6, 0), (3, 0)],
    "w64-l32t32b32-n17": [(0, 0), (1, 0), (17, 0), (16, 0), (13, 3), (10, 0), (6, 0), (3, 0)],
    "w64-l32f33t17-n64": [(0, 0), (1, 0), (64, 0), (63, 65), (57, 61), (19, 1), (25, 0), (12, 0)],
    "w64-m13-n65": [(0, 0), (1, 0), (65, 16), (64, 5), (52, 2), (39, 2), (26, 0), (13, 1)],
    "w64-m13-n80": [(0, 0), (1, 0), (48, 2, "spread"), (36, 1, "spread")],
    "w64-l32t32b32-n112": [(0, 0), (1, 0), (112, 0), (111, 0), (44, 5), (42, 2), (48, 1, 'spread'), (36, 7, 'spread')],
    "w128-f1_65-n37": [(0, 0), (1, 0), (37, 2), (36, 1), (29, 1), (22, 0), (14, 0), (7, 0)],
    "w128-f3_33-n48": [(0, 0), (1, 0), (48, 0), (47, 4), (38, 2), (28, 0), (19, 0), (9, 0)],
    "w128-max-n112": [(0, 0), (1, 0), (112, 0), (111, 0), (28, 2), (33, 1), (40, 7, 'spread'), (30, 4, 'spread')],
    "out-labels33": [(0, 0), (1, 0), (37, 6), (36, 0), (29, 0), (22, 0), (14, 0), (7, 0)],
    "out-f1_129": [(0, 0), (1, 0), (37, 0), (36, 0), (29, 0), (22, 0), (14, 0), (7, 0)],
    "out-f2_129": [(0, 0), (1, 0), (37, 0), (36, 0), (29, 2), (22, 0), (14, 0), (7, 0)],
    "out-f3_65": [(0, 0), (1, 0), (37, 2), (36, 1), (29, 1), (22, 0), (14, 0), (7, 0)],
    "out-n113": [(0, 0), (1, 0), (113, 4), (112, 5), (90, 0), (67, 0), (45, 1), (22, 0)],
    "out-k9": [(0, 0), (1, 0), (100, 3), (99, 2), (80, 3), (60, 0), (40, 0), (20, 0)],
    "out-k11": [(0, 0), (1, 0), (100, 1), (99, 1), (80, 2), (60, 0), (40, 0), (20, 0)],
    "w64-t33": [(0, 0), (1, 0), (37, 0), (36, 2), (29, 3), (22, 0), (14, 0), (7, 0)],
    "w64-b33": [(0, 0), (1, 0), (37, 0), (36, 0), (29, 1), (22, 2), (14, 6), (7, 1)],
    "plain-max-lds": [(0, 0), (1, 0), (43, 16), (42, 3), (27, 0), (25, 0), (17, 2), (8, 0)],
    "plain-max-global": [(0, 0), (1, 0), (44, 21), (43, 2), (28, 0), (26, 0), (17, 0), (8, 0)],
    "plain-max-n1024-k64": [(76, 18, 'spread'), (68, 5, 'spread')],
    "knn-n64": [(0, 0), (1, 0), (64, 26), (63, 9)],
    "knn-n65": [(0, 0), (1, 0), (65, 22), (64, 41)],
    "knn-n128": [(0, 0), (1, 0), (128, 5), (127, 12)],
    "knn-n129": [(0, 0), (1, 0), (129, 0), (128, 0)],
    "knn-n256": [(0, 0), (1, 0), (204, 4), (179, 124), (90, 1, 'spread'), (50, 0, 'spread')],
    "knn-n257": [(0, 0), (1, 0), (154, 66), (128, 11), (90, 0, 'spread'), (50, 1, 'spread')],
    "knn-n512": [(0, 0), (1, 0), (79, 0), (83, 0), (90, 0, 'spread'), (50, 0, 'spread')],
    "knn-n513": [(0, 0), (1, 0), (124, 1), (83, 0), (90, 2, 'spread'), (50, 6, 'spread')],
    "k-eq-n12": [(0, 0), (1, 0), (12, 0), (11, 0), (9, 0), (7, 0), (4, 0), (2, 0)],
    "k64-n64": [(0, 0), (1, 0), (64, 0), (63, 0), (51, 0), (38, 0), (25, 0), (12, 0)],
    "k64-n200": [(0, 0), (1, 0), (110, 2, "spread"), (100, 2)],
    "k1-n40": [(0, 0), (1, 0), (40, 0), (39, 0), (32, 0), (24, 0), (16, 0), (8, 0)],
}


def _row(rid, dims, n, k, route, g=8, seed=1, model="random"):
    fills = FILLS[rid]
    cmax = max(3, *dims[:4])
    scratch = "lds" if 4 * (n * (3 * cmax + dims[3] + 1 + k) + 64) <= LDS_SWITCH else "global"
    return dict(id=rid, dims=dims, N=n, K=k, route=route, G=g, fills=fills, seed=seed, model=model, scratch=scratch)


_FIT = plain_lds_fit(MAXM, 10)
# (labels, f1, f2, f3, T, B); N, K; the embed route the header promises; G graphs (FILLS)
EMBED_ROWS = [
    # ---- zero-padded tuned kernels
    _row("tuned-1x6-n24", (1, 1, 1, 1, 1, 1), 24, 10, "tuned"),
    _row("tuned-below-n64", (11, 63, 63, 31, 15, 15), 64, 10, "tuned"),
    # ---- two-plane embed, <64,32>: one row tile (N = K, 16), a second tile of one live row (17), the nrt > 4 sort branch at
    #      its edge (64 / 65), every row tile (112)
    _row("w64-m13-n10", M13, 10, 10, "wide64"),
    _row("w64-l32f33t17-n16", (32, 33, 64, 32, 17, 16), 16, 10, "wide64"),
    _row("w64-l32t32b32-n17", (32, 64, 64, 32, 32, 32), 17, 10, "wide64"),
    _row("w64-l32f33t17-n64", (32, 33, 64, 32, 17, 16), 64, 10, "wide64"),
    _row("w64-m13-n65", M13, 65, 10, "wide64"),
    _row("w64-m13-n80", M13, 80, 10, "wide64", g=4),      # five row tiles, the fifth full: 7 - 10 distinct nodes in it
    _row("w64-l32t32b32-n112", (32, 64, 64, 32, 32, 32), 112, 10, "wide64"),
    # ---- two-plane embed, <128,64>
    _row("w128-f1_65-n37", (12, 65, 64, 32, 16, 16), 37, 10, "wide128"),
    _row("w128-f3_33-n48", (12, 64, 64, 33, 16, 16), 48, 10, "wide128"),
    _row("w128-max-n112", (32, 128, 128, 64, 32, 32), 112, 10, "wide128"),
    # ---- one step outside each two-plane limit: the plain kernel
    _row("out-labels33", (33, 64, 64, 32, 16, 16), 37, 10, "plain"),
    _row("out-f1_129", (12, 129, 64, 32, 16, 16), 37, 10, "plain"),
    _row("out-f2_129", (12, 64, 129, 32, 16, 16), 37, 10, "plain"),
    _row("out-f3_65", (12, 64, 64, 65, 16, 16), 37, 10, "plain"),
    _row("out-n113", M13, 113, 10, "plain"),
    _row("out-k9", M13, 100, 9, "plain"),
    _row("out-k11", M13, 100, 11, "plain"),
    # ---- embed two-plane, tail plain
    _row("w64-t33", (12, 64, 64, 32, 33, 16), 37, 10, "wide64"),
    _row("w64-b33", (12, 64, 64, 32, 16, 33), 37, 10, "wide64"),
    # ---- plain fp32: the last node_num in LDS, the first in global scratch, the maximum of everything
    _row("plain-max-lds", MAXM, _FIT, 10, "plain"),
    _row("plain-max-global", MAXM, _FIT + 1, 10, "plain"),
    _row("plain-max-n1024-k64", MAXM, 1024, 64, "plain", g=2),
    # ---- knn_select_row's instances (64 candidates per lane block: 1, 2, 4, 8, 16 blocks) and the K edges, on a
    #      13-label copy of the shipped 64-wide checkpoint.  From 256 slots on a settled graph cannot be full: two spread
    #      graphs (G = 6) put distinct nodes into the last candidate blocks, slot N - 1 included
    _row("knn-n64", M13, 64, 10, "wide64", g=4, model="ckpt13"),
    _row("knn-n65", M13, 65, 10, "wide64", g=4, model="ckpt13"),
    _row("knn-n128", M13, 128, 10, "plain", g=4, model="ckpt13"),
    _row("knn-n129", M13, 129, 10, "plain", g=4, model="ckpt13"),
    _row("knn-n256", M13, 256, 10, "plain", g=6, model="ckpt13"),
    _row("knn-n257", M13, 257, 10, "plain", g=6, model="ckpt13"),
    _row("knn-n512", M13, 512, 10, "plain", g=6, model="ckpt13"),
    _row("knn-n513", M13, 513, 10, "plain", g=6, model="ckpt13"),
    _row("k-eq-n12", M13, 12, 12, "plain", model="ckpt13"),
    _row("k64-n64", M13, 64, 64, "plain", model="ckpt13"),
    _row("k64-n200", M13, 200, 64, "plain", g=4, model="ckpt13"),        # a real choice among > 64 distinct nodes
    _row("k1-n40", M13, 40, 1, "plain", model="ckpt13"),
]
_BY_ID = {r["id"]: r for r in EMBED_ROWS}
assert len(_BY_ID) == len(EMBED_ROWS)


def row_tau(row):
    """the margin a graph must keep on the route that serves the row (the bit-23 run of a two-plane row keeps the same set)"""
    return ref64.TAU_PLAIN if row["route"] == "plain" else ref64.TAU_WIDE


def one_graph(row, count, gseed, spread=False):
    """centers f32 [N,3], labels i32 [N] (-1 = pad) of one graph: `count` real nodes in label-ascending order, the last
    label channel in use; coordinates as sg_pr_amd.synth.make_graphs draws them.  The pads trail the real nodes, or, with
    `spread`, the real nodes sit at evenly spaced slots from 0 to N - 1 with the pads between them: a sparse graph (settled
    at the measured tau) whose LAST candidates are distinct real nodes that other rows must take - packed and dense input
    only, a ragged store keeps its pads at the end.  A graph depends on (row seed, N, labels, count, gseed, spread) alone."""
    n, labels = row["N"], row["dims"][0]
    rng = np.random.default_rng((1000 + row["seed"], n, labels, count, gseed))
    c = np.zeros((n, 3), dtype=np.float32)
    l = -np.ones(n, dtype=np.int32)
    if count:
        at = np.round(np.linspace(0, n - 1, count)).astype(np.int64) if spread else np.arange(count)
        assert len(set(at.tolist())) == count
        lab = rng.integers(0, labels, size=count)
        lab[0] = labels - 1
        lab.sort()
        c[at, :2] = rng.uniform(-50.0, 50.0, size=(count, 2))
        c[at, 2] = rng.uniform(-2.0, 1.0, size=count)
        l[at] = lab
    return c, l


def is_spread(fill):
    return len(fill) > 2 and fill[2] == "spread"


def make_graphs(row):
    """centers f32 [G,N,3], labels i32 [G,N] of a table row"""
    fills = row["fills"]
    assert len(fills) == row["G"] and all(0 <= f[0] <= row["N"] for f in fills)
    graphs = [one_graph(row, f[0], f[1], is_spread(f)) for f in fills]
    return np.stack([g[0] for g in graphs]), np.stack([g[1] for g in graphs])


def _args_for(dims, n, k):
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.filters_1, args.filters_2, args.filters_3, args.tensor_neurons, args.bottle_neck_neurons = dims[1:]
    args.node_num, args.K = n, k
    return args


@functools.lru_cache(maxsize=None)
def state_dict_for(dims, model="random"):
    """fp32 state dict of a model: the repository's _randomised SG, or the 13-label copy of the shipped checkpoint (one
    extra label channel with zero weights: an any-shape handle computing the checkpoint's function)"""
    if model == "ckpt13":
        from oracle import sgpr_oracle
        sd = {k: v.clone() for k, v in sgpr_oracle.load_checkpoint(os.path.join(GOLDEN, "model.pth")).items()}
        w = sd["dgcnn_f_conv1.0.weight"]
        w4 = w.reshape(w.shape[0], 2, 12)
        sd["dgcnn_f_conv1.0.weight"] = torch.cat((w4, torch.zeros(w.shape[0], 2, 1)), dim=2).reshape(w.shape[0], 26, 1, 1)
        assert dims == M13
        return sd
    from sg_pr_amd import sg_net
    from test_gpu_parity import _randomised
    torch.manual_seed(dims[0] * 1000 + dims[1] + dims[4])
    return _randomised(sg_net.SG(_args_for(dims, 64, 10), dims[0]))[1]


@functools.lru_cache(maxsize=4)
def host_case(rid):
    """the model, the graphs and the float64 reference of one table row (computed once per process)"""
    row = _BY_ID[rid]
    from sg_pr_amd import synth
    sd = state_dict_for(row["dims"], row["model"])
    c, l = make_graphs(row)
    feats = torch.from_numpy(synth.dense_features(c, l, num_labels=row["dims"][0]))
    ref = ref64.embed(ref64.state_dict_f64(sd), feats, row["K"])
    return dict(sd=sd, centers=c, labels=l, feats=feats, ref=ref)


def cap_report(row, ok):
    """the cap of the issue: at most a quarter unsettled and at least four settled; with G = 2 both settled"""
    g, n_ok = ok.numel(), int(ok.sum())
    if g == 2:
        return n_ok == 2
    return (g - n_ok) * 4 <= g and n_ok >= 4


# ------------------------------------------------------------------------------------------------------------ GPU side
gpu = pytest.mark.gpu


def _engine(dims, model="random"):
    from sg_pr_amd.engine import Engine, SgprDims
    return Engine(state_dict_for(dims, model), SgprDims(*dims))


class _plain_only:
    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.eng.set_skip_mask(PLAIN_BIT)

    def __exit__(self, *exc):
        self.eng.set_skip_mask(0)


def _ws_bytes(eng, g, n, k):
    return int(eng.lib.sgpr_embed_workspace_bytes(eng._h, g, n, k))


@gpu
@pytest.mark.parametrize("rid", [r["id"] for r in EMBED_ROWS])
def test_embed_sweep(rid):
    from sg_pr_amd.allpairs import RaggedGraphs
    from sg_pr_amd.engine import SgprError
    row = _BY_ID[rid]
    dims, n, k, g, route = row["dims"], row["N"], row["K"], row["G"], row["route"]
    labels, f3 = dims[0], dims[3]
    case = host_case(rid)
    c, l, feats, ref = case["centers"], case["labels"], case["feats"], case["ref"]
    ok = ref64.settled(ref, row_tau(row))
    assert cap_report(row, ok), (rid, ok.tolist())                    # (tests/test_any_shape_ref_host.py keeps this true)
    eng = _engine(dims, row["model"])
    try:
        # ---- the route, as far as the ABI shows it
        assert eng.any_shape == (route != "tuned") and eng.pw == (32 if route == "tuned" else f3), rid
        if route != "tuned":
            per_graph = _ws_bytes(eng, 2, n, k) - _ws_bytes(eng, 1, n, k)   # (the flag bytes of 1 and 2 graphs round alike)
            lds = eng.lds_bytes(n, k)
            fixed = eng.lds_bytes(1024, 64)                            # (no model fits there: the kernel's static part alone)
            in_global = per_graph > 0
            assert in_global == (row["scratch"] == "global"), (rid, per_graph, lds)
            assert (lds == fixed) == in_global and lds <= fixed + LDS_SWITCH, (rid, lds, fixed)
            if in_global:
                assert per_graph > LDS_SWITCH, (rid, per_graph)
            if rid in ("plain-max-lds", "plain-max-global"):           # node_num from the library's own answers
                fit = max(v for v in range(k, 200) if eng.lds_bytes(v, k) > fixed)
                assert n == fit + (rid == "plain-max-global"), (rid, n, fit)
        pooled, att, emb = eng.embed(c, l, k, want_att=True, want_emb=True)
        eng.check_status()
        runs = {"default": (pooled, att, emb)}
        if route != "tuned":
            with _plain_only(eng):
                plain = eng.embed(c, l, k, want_att=True, want_emb=True)
            two_plane = not torch.equal(plain[0], pooled)
            assert two_plane == route.startswith("wide"), (rid, route)  # bit 23 changes the bits exactly inside the limits
            if two_plane:
                runs["plain"] = plain
        # ---- every graph: finite, attention in [0, 1]
        for name, (p_, a_, e_) in runs.items():
            assert torch.isfinite(p_).all() and torch.isfinite(e_).all(), (rid, name)
            assert float(a_.min()) >= 0.0 and float(a_.max()) <= 1.0, (rid, name)
        # ---- settled graphs against the float64 reference
        sel = torch.nonzero(ok).reshape(-1)
        r_emb, r_att, r_pooled = ref["emb"][sel], ref["att"][sel], ref["pooled"][sel]
        emb_gate = EMB_GATE * max(1.0, float(r_emb.abs().max()))
        pooled_gate = POOLED_GATE * max(1.0, float(r_pooled.abs().max()))
        for name, (p_, a_, e_) in runs.items():
            d_emb = float((e_.cpu().double()[sel][..., :f3] - r_emb).abs().max())
            d_pooled = float((p_.cpu().double()[sel][:, :f3] - r_pooled).abs().max())
            d_att = float((a_.cpu().double()[sel] - r_att).abs().max())
            print("SWEEP %s %s settled %d/%d emb %.3e (gate %.3e) pooled %.3e (gate %.3e) att %.3e"
                  % (rid, name, sel.numel(), g, d_emb, emb_gate, d_pooled, pooled_gate, d_att))
            assert d_emb < emb_gate and d_pooled < pooled_gate and d_att < ATT_GATE, (rid, name, d_emb, d_pooled, d_att)
            if route == "tuned" and f3 < 32:
                assert float(p_[:, f3:].abs().max()) == 0.0, rid
        if "plain" in runs:                                            # two datapaths, and they agree
            scale = max(1.0, float(r_pooled.abs().max()))
            assert float((runs["plain"][0][sel] - pooled[sel]).abs().max()) < ROUTE_GATE * scale, rid
        # ---- the other input forms: the same bits, for every graph
        trail = [gi for gi, f in enumerate(row["fills"]) if not is_spread(f)]      # (a ragged store keeps its pads at the end)
        rag = RaggedGraphs.from_padded(c[trail], l[trail], device="cuda", num_labels=labels)
        p_r, a_r, e_r = eng.embed_ragged(rag.centers, rag.labels, rag.offsets, n, k, want_att=True, want_emb=True)
        assert torch.equal(p_r, pooled[trail]) and torch.equal(a_r, att[trail]) and torch.equal(e_r, emb[trail]), rid
        p_d, a_d, e_d = eng.embed_dense(feats, k, want_att=True, want_emb=True)
        assert torch.equal(p_d, pooled) and torch.equal(a_d, att) and torch.equal(e_d, emb), rid
        half = g // 2
        score, a1, a2 = eng.forward_dense(feats[:half], feats[half:2 * half], k)
        assert torch.equal(torch.cat((a1, a2)), att[:2 * half]), rid
        pairs = eng.score_pairs(pooled[:half].contiguous(), pooled[half:2 * half].contiguous())
        assert float((score - pairs).abs().max()) < LIST_GATE, rid
        eng.check_status()
        # ---- non-vacuity: a settled graph whose embedding varies over the nodes in at least half of the channels
        vary = ((emb[sel][..., :f3].amax(dim=1) - emb[sel][..., :f3].amin(dim=1)) > 0).sum(dim=1)
        assert int(vary.max()) * 2 >= f3, (rid, vary.tolist())
        # ---- a label the model does not have is reported
        bad = l.copy()
        bad[int(np.argmax((l >= 0).sum(axis=1))), 0] = labels
        eng.embed(c, bad, k)
        with pytest.raises(SgprError):
            eng.check_status()
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- tail
# (labels, f1, f2, f3, T, B), the route of sgpr_score_all_pairs: every tail-distinct model of the embed table, then the
# plain rectangle kernel's instance choice (T = 16 / 17, 32 / 33, 64) at f3 = 32 under one and 64 bottleneck neurons
TAIL_ROWS = [
    ("tuned-1x6", (1, 1, 1, 1, 1, 1), "tuned"),
    ("tuned-below", (11, 63, 63, 31, 15, 15), "tuned"),
    ("wide-m13", M13, "wide"),
    ("wide-t17", (32, 33, 64, 32, 17, 16), "wide"),
    ("wide-t32b32", (32, 64, 64, 32, 32, 32), "wide"),
    ("wide-f3_33", (12, 64, 64, 33, 16, 16), "wide"),
    ("wide-max", (32, 128, 128, 64, 32, 32), "wide"),
    ("plain-labels33", (33, 64, 64, 32, 16, 16), "plain"),
    ("plain-f3_65", (12, 64, 64, 65, 16, 16), "plain"),
    ("plain-t33", (12, 64, 64, 32, 33, 16), "plain"),
    ("plain-b33", (12, 64, 64, 32, 16, 33), "plain"),
    ("plain-max", MAXM, "plain"),
] + [("b1-t%d" % t, (13, 64, 64, 32, t, 1), "wide" if t <= 32 else "plain") for t in (16, 17, 32, 33, 64)] \
  + [("b64-t%d" % t, (13, 64, 64, 32, t, 64), "plain") for t in (16, 17, 32, 33, 64)]
RECT_R = (1, 16, 17, 33)
RECT_M = (1, 16, 17, 64, 65, 256, 257, 300)          # 16-column blocks, 256-column chunks / tiles and their edges


def _rect(eng, rows, cols, r, m, ld):
    """sgpr_score_all_pairs on rows[:r] x cols[:m] into a [r, ld] buffer of NaNs -> (scores [r, m], the columns past m)"""
    buf = torch.full((r, ld), float("nan"), dtype=torch.float32, device="cuda")
    eng.score_all_pairs(rows[:r].contiguous(), cols[:m].contiguous(), out=buf[:, :m])
    return buf[:, :m], buf[:, m:]


@gpu
@pytest.mark.parametrize("tid", [t[0] for t in TAIL_ROWS])
def test_tail_sweep(tid):
    from sg_pr_amd import sg_net
    _, dims, route = next(t for t in TAIL_ROWS if t[0] == tid)
    sd = state_dict_for(dims)
    sd64 = ref64.state_dict_f64(sd)
    model = sg_net.SG(_args_for(dims, 64, 10), dims[0])
    model.load_state_dict(sd)
    model.eval()
    eng = model.engine()
    try:
        _tail_case(tid, dims, route, model, eng, sd64)
    finally:
        eng.close()


def _tail_case(tid, dims, route, model, eng, sd64):
    f3, pw = dims[3], eng.pw
    assert eng.any_shape == (route != "tuned") and pw == (32 if route == "tuned" else f3), tid
    gen = torch.Generator().manual_seed(7 + f3 + dims[4])
    rmax, mmax, ld = max(RECT_R), max(RECT_M), max(RECT_M) + 9
    differs, spread, handed_over = False, 0.0, False
    for sc_ in (1.0, 0.03):
        rows = torch.zeros(rmax, pw)
        cols = torch.zeros(mmax, pw)
        rows[:, :f3] = torch.randn(rmax, f3, generator=gen) * sc_
        cols[:, :f3] = torch.randn(mmax, f3, generator=gen) * sc_
        want = ref64.tail(sd64, rows[:, :f3], cols[:, :f3])
        rows, cols = rows.cuda(), cols.cuda()
        full, past = _rect(eng, rows, cols, rmax, mmax, ld)
        assert torch.isnan(past).all(), (tid, sc_)                      # nothing is written past column M
        dev = float((full.cpu().double() - want).abs().max())
        spread = max(spread, float(full.max() - full.min()))
        print("SWEEP tail %s scale %.2f max|d| vs float64 %.3e spread %.3e" % (tid, sc_, dev, float(full.max() - full.min())))
        assert dev < SCORE_TOL, (tid, sc_, dev)
        if route != "tuned":
            with _plain_only(eng):
                full_plain, past_plain = _rect(eng, rows, cols, rmax, mmax, ld)
            assert torch.isnan(past_plain).all(), (tid, sc_)
            assert float((full_plain.cpu().double() - want).abs().max()) < SCORE_TOL, (tid, sc_)
            assert float((full - full_plain).abs().max()) < TAIL_ROUTE_GATE, (tid, sc_)
            differs = differs or not torch.equal(full, full_plain)
        # ---- every sub-rectangle: the bits of the full call, nothing past its last column
        for r in RECT_R:
            for m in RECT_M:
                sub, past = _rect(eng, rows, cols, r, m, m + 3)
                assert torch.equal(sub, full[:r, :m]) and torch.isnan(past).all(), (tid, sc_, r, m)
                if route != "tuned":
                    with _plain_only(eng):
                        sub_p, past_p = _rect(eng, rows, cols, r, m, m + 3)
                    assert torch.equal(sub_p, full_plain[:r, :m]) and torch.isnan(past_p).all(), (tid, sc_, r, m)
        # ---- the list forms on 300 random pairs of the rectangle
        rng = np.random.default_rng(f3)
        i1 = rng.integers(0, rmax, 300).astype(np.int32)
        i2 = rng.integers(0, mmax, 300).astype(np.int32)
        t1, t2 = torch.from_numpy(i1), torch.from_numpy(i2)
        at = full[t1.long().cuda(), t2.long().cuda()]
        lst = eng.score_pairs(rows, cols, t1, t2)
        pooled_api = model.score_pooled(rows, cols, t1, t2)
        walked = eng.score_pair_list(rows, cols, eng.pair_plan(i1, i2, rmax, mmax))
        assert float((lst - at).abs().max()) < LIST_GATE and float((walked - at).abs().max()) < LIST_GATE, (tid, sc_)
        assert torch.equal(pooled_api, lst), (tid, sc_)                 # (a short list: sgpr_score_pairs)
        if route == "tuned":
            assert torch.equal(walked, at), (tid, sc_)                  # (an f16 handle: the matrix's entries, sgpr.h)
        else:
            assert torch.equal(walked, lst), (tid, sc_)                 # (any-shape: the plan walked pair by pair)
        assert float((lst.cpu().double() - want[t1.long(), t2.long()]).abs().max()) < SCORE_TOL, (tid, sc_)
        diag = eng.score_pairs(rows[:rmax].contiguous(), cols[:rmax].contiguous())
        assert float((diag - torch.diagonal(full[:, :rmax])).abs().max()) < LIST_GATE, (tid, sc_)
        if route == "wide":
            # ONE column vector outside the f16 range hands the whole rectangle to the plain kernel: every other column
            # - ordinary, unsaturated scores - then carries the plain kernel's bits, not the matrix cores'
            odd = cols.clone()
            odd[5, :f3] = torch.where(odd[5, :f3] >= 0, 1.0, -1.0) * 1e5
            keep = [j for j in range(mmax) if j != 5]
            got = eng.score_all_pairs(rows[:17].contiguous(), odd)
            with _plain_only(eng):
                plain_odd = eng.score_all_pairs(rows[:17].contiguous(), odd)
            assert torch.equal(got, plain_odd) and torch.isfinite(got).all(), (tid, sc_)
            assert torch.equal(got[:, keep], full_plain[:17][:, keep]), (tid, sc_)
            handed_over = handed_over or not torch.equal(got[:, keep], full[:17][:, keep])
    assert spread > 1e-3, (tid, spread)                                 # (not only saturated scores)
    assert differs == (route == "wide"), (tid, route)                   # bit 23 changes the bits exactly on the matrix-core tail
    assert handed_over == (route == "wide"), tid                        # (the hand-over is visible in unsaturated scores)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- limits
_LIMITS = (64, 256, 256, 128, 64, 64)
_NAMES = ("labels", "filters_1", "filters_2", "filters_3", "tensor", "bottleneck")


@gpu
@pytest.mark.parametrize("which", range(6), ids=_NAMES)
@pytest.mark.parametrize("value", ["limit+1", "zero"])
def test_dims_outside_the_limits_are_refused(which, value):
    from sg_pr_amd.engine import Engine, SgprDims, SgprError
    dims = list(M13)
    dims[which] = _LIMITS[which] + 1 if value == "limit+1" else 0
    blob = np.zeros(16, dtype=np.float32)
    with pytest.raises(SgprError, match="SGPR_E_DIMS"):
        Engine(blob, SgprDims(*dims))
    if value == "zero":
        return
    ok = list(M13)
    ok[which] = _LIMITS[which]                                           # (the limit itself is served)
    from sg_pr_amd import sg_net
    from test_gpu_parity import _randomised
    eng = _randomised(sg_net.SG(_args_for(tuple(ok), 16, 10), ok[0]))[0].engine()
    assert eng.any_shape
    eng.close()


@gpu
def test_node_and_k_limits_on_an_any_shape_handle():
    from sg_pr_amd.engine import SgprError
    eng = _engine(M13, "ckpt13")
    try:
        for n, k, code in ((1025, 10, "SGPR_E_NODES"), (100, 65, "SGPR_E_K"), (12, 13, "SGPR_E_K")):
            c = np.zeros((2, n, 3), dtype=np.float32)
            l = -np.ones((2, n), dtype=np.int32)
            with pytest.raises(SgprError, match=code):
                eng.embed(c, l, k)
            feats = torch.zeros(1, 3 + 13, n)
            with pytest.raises(SgprError, match=code):
                eng.forward_dense(feats, feats, k)
        # the limits themselves are served
        c, l = np.zeros((1, 1024, 3), dtype=np.float32), -np.ones((1, 1024), dtype=np.int32)
        assert torch.isfinite(eng.embed(c, l, 64)[0]).all()
        eng.check_status()
    finally:
        eng.close()
