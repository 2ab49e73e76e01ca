"""tests/any_shape_ref.py on the CPU: it agrees with the oracle wherever the oracle is defined, its neighbour rule does what
the library documents on cases small enough to check by hand, and every row of the GPU sweep's table keeps the cap on
unsettled graphs (tests/test_gpu_any_shape_sweep.py relies on it)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import any_shape_ref as ref64   # noqa: E402
import test_gpu_any_shape_sweep as sweep   # noqa: E402

INF = float("inf")


def _classes(x):
    """every feature row of x [C,N] -> the lowest index among its copies"""
    return torch.argmax(ref64.copies(x).to(torch.int8), dim=1)


@pytest.mark.parametrize("which", ["checkpoint", "random-narrow", "random-wide"])
def test_agrees_with_the_oracle_where_the_oracle_is_defined(which, oracle, oracle_sd):
    """graphs with at least K pads and settled margins: torch.topk has no choice to make, so the float64 oracle IS the
    reference (1e-12, the same neighbour sets up to identical rows) and the fp32 oracle meets the project's gates"""
    from sg_pr_amd import synth
    from test_gpu_parity import _label_sorted_graphs
    if which == "checkpoint":
        dims, sd = (12, 64, 64, 32, 16, 16), oracle_sd
    else:
        dims = (13, 64, 64, 32, 16, 16) if which == "random-narrow" else (25, 80, 112, 48, 24, 20)
        sd = sweep.state_dict_for(dims)
    n, k = 48, 10
    c, l = _label_sorted_graphs(12, n, n // 3, n - k, dims[0], seed=dims[0] + dims[3])
    feats = torch.from_numpy(synth.dense_features(c, l, num_labels=dims[0]))
    sd64 = ref64.state_dict_f64(sd)
    ref = ref64.embed(sd64, feats, k)
    ok = ref64.settled(ref, ref64.TAU_PLAIN)
    assert int(ok.sum()) >= 8, ok.tolist()
    feats, sel = feats[ok], torch.nonzero(ok).reshape(-1)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)            # (oracle.score_all_pairs allocates its result in the default dtype)
    try:
        emb64, layers64 = oracle.conv_pass(sd64, feats.double(), k, want_layers=True)
        pooled64, att64 = oracle.embed(sd64, feats.double(), k)[:2]
        mat64 = oracle.score_all_pairs(sd64, pooled64, pooled64)
    finally:
        torch.set_default_dtype(old)
    assert mat64.dtype == torch.float64
    for name in ref64.LAYERS:
        want = layers64[name]
        assert float((ref["layers"][name][sel] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
        theirs = oracle.knn(ref["inputs"][name][sel], k)
        for gi, g in enumerate(sel.tolist()):
            cls = _classes(ref["inputs"][name][g])
            a = torch.sort(cls[ref["idx"][name][g]], dim=1)[0]
            b = torch.sort(cls[theirs[gi]], dim=1)[0]
            assert torch.equal(a, b), (name, g)
    assert float((ref["emb"][sel] - emb64).abs().max()) <= 1e-12 * max(1.0, float(emb64.abs().max()))
    assert float((ref["pooled"][sel] - pooled64).abs().max()) <= 1e-12 * max(1.0, float(pooled64.abs().max()))
    assert float((ref["att"][sel] - att64).abs().max()) <= 1e-12
    assert float((ref64.tail(sd64, pooled64, pooled64) - mat64).abs().max()) <= 1e-12
    # the fp32 oracle, to the project's gates (tests/test_gpu_parity.py)
    emb32 = oracle.conv_pass(sd, feats, k)
    pooled32, att32 = oracle.embed(sd, feats, k)[:2]
    assert float((emb32.double() - emb64).abs().max()) < 1e-4 * max(1.0, float(emb64.abs().max()))
    assert float((pooled32.double() - pooled64).abs().max()) < 2e-4 * max(1.0, float(pooled64.abs().max()))
    assert float((att32.double() - att64).abs().max()) < 1e-4
    mat32 = oracle.score_all_pairs(sd, pooled32, pooled32)
    assert float((mat32.double() - mat64).abs().max()) < 1e-4


def _onehot(labels, num):
    x = torch.zeros(num, len(labels), dtype=torch.float64)
    for i, lab in enumerate(labels):
        if lab >= 0:
            x[lab, i] = 1.0
    return x


def test_full_graph_ties_across_labels_take_the_lowest_indices():
    """one-hot rows of a graph without padding: same label at distance 0, EVERY other label at distance 2"""
    idx, margin = ref64.select(_onehot([0, 0, 1, 1, 2, 2, 3, 3], 4), 4)
    assert idx[0].tolist() == [0, 1, 2, 3] and idx[3].tolist() == [2, 3, 0, 1] and idx[7].tolist() == [6, 7, 0, 1]
    assert idx[4].tolist() == [4, 5, 0, 1]
    assert (margin == 0).all()        # (the first label left out ties with the last one taken, and is another row)
    # three of a label, K = 2: the cut falls between identical rows - no choice at all; the next distance is 2, S = 1 + 1
    idx, margin = ref64.select(_onehot([0, 0, 0, 1], 2), 2)
    assert idx[0].tolist() == [0, 1] and idx[2].tolist() == [0, 1] and idx[3].tolist() == [3, 0]
    assert margin[:3].tolist() == [1.0, 1.0, 1.0]
    assert margin[3] == INF           # (row 3: nodes 0, 1, 2 tie and two are left out - copies of the taken one, and nothing else)
    idx, margin = ref64.select(_onehot([0, 0, 0, 1], 2), 3)
    assert idx[3].tolist() == [3, 0, 1] and margin[3] == INF


def test_all_padding_single_node_and_k_equal_n():
    idx, margin = ref64.select(torch.zeros(5, 7, dtype=torch.float64), 3)
    assert idx.tolist() == [[0, 1, 2]] * 7 and (margin == INF).all()
    # one real node ahead of six pads: the pads are copies of each other, the real node is one step away
    x = _onehot([2, -1, -1, -1, -1, -1, -1], 5)
    idx, margin = ref64.select(x, 3)
    assert idx[0].tolist() == [0, 1, 2] and idx[1].tolist() == [1, 2, 3] and idx[6].tolist() == [1, 2, 3]
    assert margin[0] == INF and margin[1:].tolist() == [1.0] * 6          # (pads: the real node is next, distance 1, S = 0 + 1)
    idx, margin = ref64.select(torch.randn(3, 6, dtype=torch.float64), 6)
    assert torch.equal(torch.sort(idx, dim=1)[0], torch.arange(6).repeat(6, 1)) and (margin == INF).all()
    assert idx[:, 0].tolist() == list(range(6))                           # (self first)
    # ... and through the whole reference: finite, attention in [0, 1], pooled = sum of att * emb
    sd64 = ref64.state_dict_f64(sweep.state_dict_for(sweep.M13))
    feats = torch.zeros(2, 16, 12)
    feats[1, :3, 0] = torch.tensor([3.0, -4.0, 0.5])
    feats[1, 3 + 12, 0] = 1.0
    out = ref64.embed(sd64, feats, 10)
    assert torch.isfinite(out["emb"]).all() and float(out["att"].min()) >= 0 and float(out["att"].max()) <= 1
    assert ref64.settled(out, ref64.TAU_WIDE).all()
    assert float((out["pooled"] - torch.einsum("gn,gnf->gf", out["att"], out["emb"])).abs().max()) < 1e-12
    assert float((out["emb"][0] - out["emb"][0][:1]).abs().max()) == 0    # (all padding: every row the same)


def _fake(margins):
    ref = {"emb": torch.zeros(1, 1, 1), "margins": {n: torch.full((1, 4), INF, dtype=torch.float64) for n in ref64.LAYERS}}
    for name, m in margins.items():
        ref["margins"][name] = m.reshape(1, -1)
    return ref


def test_planted_near_tie_unsettles_and_a_clear_gap_does_not():
    near = torch.tensor([[0.0, 1.0, 1.0 + 1e-9, 5.0]], dtype=torch.float64)
    idx, margin = ref64.select(near, 2)
    assert idx[0].tolist() == [0, 1] and 0 < float(margin[0]) < 1e-9      # ((1 + 1e-9)^2 - 1) / (0 + 25)
    assert not ref64.settled(_fake({"xyz2": margin}), ref64.TAU_PLAIN)[0]
    clear = torch.tensor([[0.0, 1.0, 3.0, 9.0]], dtype=torch.float64)
    idx, margin = ref64.select(clear, 2)
    assert idx[0].tolist() == [0, 1] and float(margin.min()) > 1e-2
    assert ref64.settled(_fake({"xyz2": margin}), ref64.TAU_WIDE)[0]
    # an exact tie between different rows is legal in sem1 alone
    zero = torch.tensor([0.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    assert ref64.settled(_fake({"sem1": zero}), ref64.TAU_WIDE)[0]
    assert not ref64.settled(_fake({"sem2": zero}), ref64.TAU_PLAIN)[0]
    assert not ref64.settled(_fake({"sem1": torch.full((4,), ref64.TAU_PLAIN / 2, dtype=torch.float64)}), ref64.TAU_PLAIN)[0]


@pytest.mark.parametrize("rid", [r["id"] for r in sweep.EMBED_ROWS])
def test_every_sweep_row_keeps_the_cap(rid):
    """at most a quarter of a row's graphs unsettled and at least four settled (G = 2: both); exact ties only in sem1;
    the recorded e32 covers the row's inputs (another BLAS may sum in another order: a factor of two, inside tau's 16)"""
    row = sweep._BY_ID[rid]
    case = sweep.host_case(rid)
    ok = ref64.settled(case["ref"], sweep.row_tau(row))
    assert sweep.cap_report(row, ok), (rid, ok.tolist())
    assert ref64.exact_ties_outside_sem1(case["ref"]) == 0, rid
    assert ref64.key_error_fp32(case["ref"]) <= 2 * ref64.E32, rid
    fills = (case["labels"] >= 0).sum(axis=1).tolist()
    assert fills == [f[0] for f in row["fills"]] and len(set(row["fills"])) == row["G"], rid
    for gi, f in enumerate(row["fills"]):
        if sweep.is_spread(f):                  # a distinct real node in the last slot, for a settled graph
            assert case["labels"][gi, -1] >= 0 and ok[gi], (rid, gi)
    if row["G"] >= 4:
        assert 0 in fills and 1 in fills, rid                               # an all-padding graph and a single real node
    if row["G"] == 8:
        assert row["N"] in fills and row["N"] - 1 in fills, rid             # no padding at all, and one pad
    assert int(case["labels"].max()) == row["dims"][0] - 1, rid             # labels reach the last channel


def test_the_table_names_every_boundary():
    """the shapes the issue lists, by what the header's limits say about them (the GPU test asserts the route itself)"""
    rows = sweep.EMBED_ROWS
    wide = [r for r in rows if r["route"].startswith("wide")]
    assert all(r["K"] == 10 and r["N"] <= 112 and r["dims"][0] <= 32 and max(r["dims"][1:3]) <= 128 and r["dims"][3] <= 64
               for r in wide)
    assert {r["N"] for r in rows if r["route"] == "wide64" and r["model"] == "random"} >= {10, 16, 17, 64, 65, 112}
    outside = [r for r in rows if r["id"].startswith("out-")]
    assert sorted((r["dims"][0] > 32, r["dims"][1] > 128, r["dims"][2] > 128, r["dims"][3] > 64, r["N"] > 112, r["K"])
                  for r in outside) == sorted([(True, False, False, False, False, 10), (False, True, False, False, False, 10),
                                               (False, False, True, False, False, 10), (False, False, False, True, False, 10),
                                               (False, False, False, False, True, 10), (False, False, False, False, False, 9),
                                               (False, False, False, False, False, 11)])
    fit = sweep.plain_lds_fit(sweep.MAXM, 10)
    assert {(r["N"], r["scratch"]) for r in rows if r["dims"] == sweep.MAXM} == {(fit, "lds"), (fit + 1, "global"), (1024, "global")}
    assert {r["N"] for r in rows if r["id"].startswith("knn-")} == {64, 65, 128, 129, 256, 257, 512, 513}
    assert {(r["N"], r["K"]) for r in rows if r["id"].startswith("k")} >= {(12, 12), (64, 64), (40, 1)}
