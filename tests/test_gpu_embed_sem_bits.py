"""The super-node (semantic) branch and the per-node GEMM walks keep their bits over the label histograms that steer them:
`pooled`, `att` and `emb` of a pool of graphs with EXPLICIT labels equal, word for word, what
tests/golden/embed_sem_bits.npz recorded from the library BEFORE the branch's two layers became streams of constant shape and
the GEMMs' row-tile walks were merged.  (tests/test_gpu_embed_bits.py draws its labels from one histogram; the branch sees a graph
only through "how many nodes carry label v", so this pool varies exactly that.)

The lean pool (node_num 100, K 10; processed slots = real nodes + the representative of the padding slots):
  one label only, with >= K nodes;  twelve labels x 3 nodes;  twelve labels x 1 node;
  labels with exactly K-1, K and K+1 nodes in one graph (the `count < K` boundary, on rows and on candidates), twice:
    in the middle of the label range and on labels 0 / 11;
  six labels with exactly K nodes and six absent;  a label present only as the last real node;
  graphs of 16, 17, 32, 33, 48, 49 and 64 processed slots (the one- to four-row-tile walks of the per-node GEMMs).
Launches: every graph alone, batches of 5 (split launch: the one-wave form of the branch), a batch of 300 drawn from the
pool (throughput plan); each plain, with `order` + `node_cap`, and with `node_cap` alone.
The big pool (node_num 256, K 20): three graphs in a launch of 300, plain and ordered - the owned-rows instance shares the
branch with K = 20.

`python tests/test_gpu_embed_sem_bits.py --record [FILE]` rewrites the fixture from the library in use (and checks that
library against itself the same way)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, NODE_NUM = 10, 100
K_BIG, NODE_NUM_BIG = 20, 256
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embed_sem_bits.npz")

# label -> node count of the graphs with a stated histogram; the slot-count graphs draw theirs (seeded)
HISTOGRAMS = (
    {3: 20},                                                # one label only, >= K nodes
    {v: 3 for v in range(12)},                              # twelve labels x 3
    {v: 1 for v in range(12)},                              # twelve labels x 1
    {2: K - 1, 5: K, 7: K + 1},                             # the count < K boundary
    {0: K + 1, 6: K, 11: K - 1},                            # ... on the first and the last label
    {v: K for v in (0, 2, 4, 6, 8, 10)},                    # six labels x K, six absent
    {1: 12, 4: 13, 11: 1},                                  # label 11 only as the last real node
)
SLOT_GRAPHS = (16, 17, 32, 33, 48, 49, 64)
BIG_HISTOGRAMS = (
    {0: K_BIG - 1, 3: K_BIG, 5: 60, 7: K_BIG + 1, 11: 1},   # the boundary at K = 20; label 11 on the last node
    {v: 10 for v in range(12)},                             # every label below K
    {9: 150},                                               # one label only
)


def _graph(hist, node_num, seed):
    """centres (seeded) + labels (ascending, as the shipped graphs list them) of one graph with the label histogram `hist`"""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.full(n, v, np.int32) for v, n in sorted(hist.items())])
    n = len(lab)
    c = np.zeros((node_num, 3), np.float32)
    c[:n, :2] = rng.uniform(-50.0, 50.0, size=(n, 2))
    c[:n, 2] = rng.uniform(-2.0, 1.0, size=n)
    l = -np.ones(node_num, np.int32)
    l[:n] = lab
    return c, l


def make_pool():
    """-> centers f32 [14, 100, 3], labels i32 [14, 100], processed slots [14]"""
    from sg_pr_amd.engine import Engine
    graphs = [_graph(h, NODE_NUM, 7000 + q) for q, h in enumerate(HISTOGRAMS)]
    for q, slots in enumerate(SLOT_GRAPHS):
        lab = np.random.default_rng(7100 + q).integers(0, 12, size=slots - 1)
        graphs.append(_graph({int(v): int(n) for v, n in zip(*np.unique(lab, return_counts=True))}, NODE_NUM, 7200 + q))
    centers, labels = np.stack([g[0] for g in graphs]), np.stack([g[1] for g in graphs])
    slots = Engine.processed_slots(centers, labels, K).numpy()
    want = np.array([sum(h.values()) + 1 for h in HISTOGRAMS] + list(SLOT_GRAPHS))
    assert np.array_equal(slots, want), slots
    return centers, labels, slots


def make_big_pool():
    """-> centers f32 [3, 256, 3], labels i32 [3, 256], processed slots [3]"""
    from sg_pr_amd.engine import Engine
    graphs = [_graph(h, NODE_NUM_BIG, 7300 + q) for q, h in enumerate(BIG_HISTOGRAMS)]
    centers, labels = np.stack([g[0] for g in graphs]), np.stack([g[1] for g in graphs])
    slots = Engine.processed_slots(centers, labels, K_BIG).numpy()
    assert np.array_equal(slots, np.array([sum(h.values()) + 1 for h in BIG_HISTOGRAMS])), slots
    return centers, labels, slots


def launches(n):
    """[(name, pool indices of the batch)]: every graph alone, fives, the batch of 300"""
    out = [("one_%d" % i, np.array([i])) for i in range(n)]
    out += [("five_a", np.arange(0, 5)), ("five_b", np.arange(5, 10)), ("five_c", np.array([10, 11, 12, 13, 2]))]
    rng = np.random.default_rng(301)
    out.append(("batch300", np.concatenate([rng.permutation(n) for _ in range(300 // n + 1)])[:300]))
    return out


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _three_ways(eng, centers, labels, slots, k, name, idx, out):
    import torch
    c = torch.from_numpy(centers[idx]).cuda()
    l = torch.from_numpy(labels[idx]).cuda()
    r = eng.embed(c, l, k, want_att=True, want_emb=True, auto_order=False)
    eng.check_status()
    out.append((name + "/plain", idx) + tuple(_bits(t) for t in r))
    order, cap = eng.size_order(c, l, k)
    assert cap == int(slots[idx].max())
    r = eng.embed(c, l, k, want_att=True, want_emb=True, node_cap=cap, order=order)
    eng.check_status()
    out.append((name + "/ordered", idx) + tuple(_bits(t) for t in r))
    r = eng.embed(c, l, k, want_att=True, want_emb=True, node_cap=cap, auto_order=False)
    eng.check_status()
    out.append((name + "/capped", idx) + tuple(_bits(t) for t in r))


def run_all(eng):
    """-> (lean launches, big launches), each [(name, pool indices, pooled, att, emb)] as raw uint32"""
    centers, labels, slots = make_pool()
    lean = []
    for name, idx in launches(len(slots)):
        _three_ways(eng, centers, labels, slots, K, name, idx, lean)
    centers, labels, slots = make_big_pool()
    big = []
    idx = np.random.default_rng(302).permutation(np.arange(300) % len(slots))
    _three_ways(eng, centers, labels, slots, K_BIG, "big300", idx, big)
    return lean, big


def compare(results, pooled, att, emb):
    """names of the launches / outputs that differ from the recorded rows in any word"""
    bad = []
    for name, idx, p, a, e in results:
        for what, got, want in (("pooled", p, pooled), ("att", a, att), ("emb", e, emb)):
            if got.shape != want[idx].shape or not np.array_equal(got, want[idx]):
                rows = sorted(set(int(i) for i, g, w in zip(idx, got, want[idx]) if not np.array_equal(g, w)))
                bad.append("%s %s (pool graphs %s)" % (name, what, rows))
    return bad


def make_engine():
    from sg_pr_amd import engine
    from oracle import sgpr_oracle
    golden = os.path.dirname(FIXTURE)
    return engine.Engine(sgpr_oracle.load_checkpoint(os.path.join(golden, "model.pth")), device=0)


@pytest.fixture(scope="module")
def results():
    eng = make_engine()
    try:
        return run_all(eng)
    finally:
        eng.close()


def test_every_launch_shape_keeps_the_recorded_bits(results):
    f = np.load(FIXTURE)
    n = len(HISTOGRAMS) + len(SLOT_GRAPHS)
    assert f["pooled"].dtype == np.uint32 and f["pooled"].shape == (n, 32)
    assert f["pooled_big"].dtype == np.uint32 and f["pooled_big"].shape == (len(BIG_HISTOGRAMS), 32)
    bad = compare(results[0], f["pooled"], f["att"], f["emb"])
    bad += compare(results[1], f["pooled_big"], f["att_big"], f["emb_big"])
    assert not bad, "\n".join(bad)


def test_recorded_rows_are_finite_and_distinct():
    """the fixture is not a row of NaNs or one graph seventeen times (either would make the comparison above hollow)"""
    f = np.load(FIXTURE)
    for sfx in ("", "_big"):
        pooled = f["pooled" + sfx]
        assert np.isfinite(pooled.view(np.float32)).all() and np.isfinite(f["emb" + sfx].view(np.float32)).all()
        assert len({row.tobytes() for row in pooled}) == len(pooled)
        att = f["att" + sfx].view(np.float32)
        assert (att >= 0).all() and (att <= 1).all() and att.std() > 0.05


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, "usage: python tests/test_gpu_embed_sem_bits.py --record [FILE]"
    FIXTURE_OUT = sys.argv[2] if len(sys.argv) == 3 else FIXTURE
    eng = make_engine()
    lean, big = run_all(eng)
    eng.close()
    rows = {}
    for sfx, res, first_name in (("", lean, "batch300/plain"), ("_big", big, "big300/plain")):
        first = next(r for r in res if r[0] == first_name)
        n = int(first[1].max()) + 1
        where = np.array([int(np.flatnonzero(first[1] == i)[0]) for i in range(n)])
        rows["pooled" + sfx], rows["att" + sfx], rows["emb" + sfx] = first[2][where], first[3][where], first[4][where]
    bad = compare(lean, rows["pooled"], rows["att"], rows["emb"]) + compare(big, rows["pooled_big"], rows["att_big"], rows["emb_big"])
    print("\n".join(bad) if bad else "every launch agrees with the recorded rows")
    if bad:
        sys.exit(1)
    np.savez_compressed(FIXTURE_OUT, **rows)
    print("wrote", FIXTURE_OUT, os.path.getsize(FIXTURE_OUT), "bytes")
