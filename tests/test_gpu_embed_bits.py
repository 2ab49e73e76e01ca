"""The lean embed kernels keep their bits: `pooled`, `att` and `emb` of a fixed pool of seeded graphs (node_num 100, K 10)
equal, word for word, what tests/golden/embed_lean_bits.npz recorded from the library BEFORE the lean instance's scalar
instruction stream was reworked - in every launch shape that reaches the lean instances, and in the debug-dump instance.

The pool (3 seeds x 11 graphs):
  processed slots 17, 32, 33, 47, 48, 49, 63, 64 - the row-tile boundaries and the 48- / 64-row variant boundary,
  one graph with two identical nodes (tied keys across the K-th place of every row that reaches them),
  one graph with fewer than K padding slots (no representative: the second pass embeds it),
  one graph whose coordinates exceed the f16 range (flagged and embedded again by the wide-range instance).
Launches: single graphs and batches of 5 (split launch), a batch of 300 drawn from the pool (throughput plan); each plain
and with `order` / `node_cap`, the promised launches also on the graphs of <= 48 and <= 64 slots alone so that the 48- and
the 64-row instances run under a promise.  A graph's result is a function of the graph alone, so every launch is held
against the same 33 recorded rows.

`python tests/test_gpu_embed_bits.py --record` rewrites the fixture from the library in use (and checks that library
against itself the same way)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
NODE_NUM = 100
SLOTS = (17, 32, 33, 47, 48, 49, 63, 64)
SEEDS = (0, 1, 2)
PER_SEED = len(SLOTS) + 3
TIE, FEW_PAD, WIDE = len(SLOTS), len(SLOTS) + 1, len(SLOTS) + 2       # places within a seed's 11 graphs
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embed_lean_bits.npz")


def make_pool():
    """-> centers f32 [33, 100, 3], labels i32 [33, 100], processed slots [33]"""
    from sg_pr_amd import synth
    from sg_pr_amd.engine import Engine
    cs, ls = [], []
    for seed in SEEDS:
        for q, slots in enumerate(SLOTS):
            # slots - 1 nodes + the representative of the (>= K) padding slots
            c, l, _ = synth.make_graphs(1, NODE_NUM, slots - 1, slots - 1, 1000 * seed + q, kitti_like=True)
            cs.append(c[0])
            ls.append(l[0])
        c, l, _ = synth.make_graphs(1, NODE_NUM, 40, 40, 1000 * seed + 100, kitti_like=True)
        c[0, 7], l[0, 7] = c[0, 6], l[0, 6]                              # two identical nodes
        cs.append(c[0])
        ls.append(l[0])
        c, l, _ = synth.make_graphs(1, NODE_NUM, 95, 95, 1000 * seed + 101, kitti_like=True)   # 5 < K padding slots
        cs.append(c[0])
        ls.append(l[0])
        c, l, _ = synth.make_graphs(1, NODE_NUM, 40, 40, 1000 * seed + 102, kitti_like=True)
        cs.append(c[0] * np.float32(2000.0))                             # coordinates up to 1e5: beyond the f16 range
        ls.append(l[0])
    centers, labels = np.stack(cs).astype(np.float32), np.stack(ls).astype(np.int32)
    slots = Engine.processed_slots(centers, labels, K).numpy()
    want = np.array((list(SLOTS) + [41, NODE_NUM, 41]) * len(SEEDS))
    assert np.array_equal(slots, want), slots
    return centers, labels, slots


def launches(slots):
    """[(name, pool indices of the batch)]: single graphs, fives, the batch of 300, the <= 48 / <= 64 slot subsets"""
    out = [("one_%d" % i, np.array([i])) for i in range(PER_SEED)]
    out += [("five_a", np.arange(0, 5)), ("five_b", np.arange(5, 10)), ("five_c", np.array([10, 3, 8, 9, 7]))]
    rng = np.random.default_rng(300)
    big = np.concatenate([rng.permutation(len(slots)) for _ in range(10)])[:300]
    out.append(("batch300", big))
    out.append(("batch300_le48", big[slots[big] <= 48]))
    out.append(("batch300_le64", big[slots[big] <= 64]))
    return out


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def run_all(eng):
    """every launch -> [(name, pool indices, pooled, att, emb)] as raw uint32"""
    import torch
    centers, labels, slots = make_pool()
    out = []
    for name, idx in launches(slots):
        c = torch.from_numpy(centers[idx]).cuda()
        l = torch.from_numpy(labels[idx]).cuda()
        r = eng.embed(c, l, K, want_att=True, want_emb=True, auto_order=False)
        eng.check_status()
        out.append((name + "/plain", idx) + tuple(_bits(t) for t in r))
        order, cap = eng.size_order(c, l, K)
        assert cap == int(slots[idx].max())
        r = eng.embed(c, l, K, want_att=True, want_emb=True, node_cap=cap, order=order)
        eng.check_status()
        out.append((name + "/ordered", idx) + tuple(_bits(t) for t in r))
        r = eng.embed(c, l, K, want_att=True, want_emb=True, node_cap=cap, auto_order=False)
        eng.check_status()
        out.append((name + "/capped", idx) + tuple(_bits(t) for t in r))
    r = eng.embed(centers, labels, K, debug=True)[:3]
    eng.check_status()
    out.append(("pool/debug", np.arange(len(slots))) + tuple(_bits(t) for t in r))
    return out


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
    assert f["pooled"].dtype == np.uint32 and f["pooled"].shape == (PER_SEED * len(SEEDS), 32)
    bad = compare(results, f["pooled"], f["att"], f["emb"])
    assert not bad, "\n".join(bad)


def test_recorded_rows_are_finite_and_distinct(results):
    """the fixture is not a row of NaNs or one graph thirty-three times (either would make the comparison above hollow)"""
    f = np.load(FIXTURE)
    pooled = f["pooled"].view(np.float32)
    assert np.isfinite(pooled).all() and np.isfinite(f["emb"].view(np.float32)).all()
    assert len({row.tobytes() for row in f["pooled"]}) == len(pooled)
    att = f["att"].view(np.float32)                       # a sigmoid: in fp32 it reaches 0 and 1 (the wide-range graphs do)
    assert (att >= 0).all() and (att <= 1).all() and att.std() > 0.05


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, "usage: python tests/test_gpu_embed_bits.py --record [FILE]"
    if len(sys.argv) == 3:
        FIXTURE_OUT = sys.argv[2]
    else:
        FIXTURE_OUT = FIXTURE
    eng = make_engine()
    res = run_all(eng)
    eng.close()
    first = next(r for r in res if r[0] == "batch300/plain")
    n = PER_SEED * len(SEEDS)
    where = np.array([int(np.flatnonzero(first[1] == i)[0]) for i in range(n)])
    pooled, att, emb = first[2][where], first[3][where], first[4][where]
    bad = compare(res, pooled, att, emb)
    print("\n".join(bad) if bad else "every launch agrees with the recorded rows")
    if bad:
        sys.exit(1)
    np.savez_compressed(FIXTURE_OUT, pooled=pooled, att=att, emb=emb)
    print("wrote", FIXTURE_OUT, os.path.getsize(FIXTURE_OUT), "bytes")
