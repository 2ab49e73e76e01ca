"""Upstream graph generation on the GPU (sgpr_cluster_scan / sgpr_graph_edges) against the oracle's
restatement of gen_label_graph.py:196-398.  `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest
import torch

import cluster_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def go():
    from oracle import graph_oracle
    return graph_oracle


@pytest.mark.parametrize("seed,scale", [(0, 0.5), (1, 1.0)])
def test_scan_to_nodes_matches_oracle(go, seed, scale):
    from sg_pr_amd import synth, gen_label_graph as glg
    pts, lab = synth.labelled_scan(seed=seed, scale=scale)
    want_cl = go.gen_labels(pts, lab)
    want = go.gen_graphs(want_cl)
    sc = glg.cluster_scan(pts, lab)
    got = glg.gen_graphs(sc)
    # integer outputs bit-exact: node labels in the reference's order, cluster sizes, every point's cluster
    assert got["nodes"] == want["nodes"] and len(got["nodes"]) >= 20
    inst = want_cl[:, 5].astype(int)
    node_inst = [i for i in np.unique(inst) if int(want_cl[inst == i][0, 4]) not in (9, 10)]
    np.testing.assert_array_equal(sc.node_sizes.cpu().numpy(), [int((inst == i).sum()) for i in node_inst])
    # centres: the oracle averages float64 copies of the float32 coordinates; the kernel sums 2^-24 m fixed point
    np.testing.assert_allclose(np.array(got["centers"]), np.array(want["centers"]), rtol=0, atol=1e-6)
    # ... and that makes them reproducible bit for bit: the exact reference (tests/cluster_ref.py)
    exact = cluster_ref.cluster_ref(pts, lab)
    np.testing.assert_array_equal(sc.centers.cpu().numpy().view(np.int64), exact["centers"].view(np.int64))
    np.testing.assert_array_equal(sc.point_node.cpu().numpy(), exact["point_node"])
    # the reference's intermediate cluster array, up to the order of the rows inside a cluster
    got_cl = glg.gen_labels(pts, lab)
    assert got_cl.shape == want_cl.shape

    def canon(a):
        return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0], a[:, 5]))]
    np.testing.assert_array_equal(canon(got_cl), canon(want_cl))
    # edges of gen_graphs (dead weight for the scorer, part of the reference's JSON)
    assert got["edges"] == want["edges"] and len(got["edges"]) > 0
    np.testing.assert_allclose(got["weights"], want["weights"], rtol=0, atol=1e-9)


def test_cluster_scan_properties_and_edges_of_the_input_space(go):
    from sg_pr_amd import synth, gen_label_graph as glg, engine
    pts, lab = synth.labelled_scan(seed=2, scale=0.5)
    base = glg.cluster_scan(pts, lab)
    # 1. the node set does not depend on the point order; two runs are bit-identical (integer centroid sums)
    again = glg.cluster_scan(pts, lab)
    assert torch.equal(base.centers, again.centers) and torch.equal(base.point_node, again.point_node)
    perm = np.random.default_rng(5).permutation(len(lab))
    sh = glg.cluster_scan(pts[perm], lab[perm])

    def key(s):
        return sorted(zip(s.node_labels.cpu().tolist(), s.node_sizes.cpu().tolist(), map(tuple, s.centers.cpu().tolist())))
    assert key(base) == key(sh)                                  # same labels, sizes AND bit-identical centres
    # 2. xyz-only points (stride 3) give the same clusters as xyzr (stride 4)
    s3 = glg.ScanClusters(None, None, *engine.cluster_scan(torch.from_numpy(np.ascontiguousarray(pts[:, :3])).cuda(),
                                                           torch.from_numpy(lab.view(np.int32)).cuda(), want_point_node=True))
    assert torch.equal(s3.centers, base.centers) and torch.equal(s3.point_node, base.point_node)
    # 3. empty scan, and a scan of discarded classes only
    e = glg.cluster_scan(np.zeros((0, 4), np.float32), np.zeros(0, np.uint32))
    assert len(e) == 0
    d = glg.cluster_scan(pts[:500], np.full(500, 30, np.uint32))
    assert len(d) == 0 and (d.point_node.cpu().numpy() == -1).all()
    # 4. a cluster above PCL's maximum size (50 000 points) is dropped, like extractEuclideanClusters does
    rng = np.random.default_rng(0)
    big = np.concatenate((rng.random((50500, 3)) * [60, 60, 0.2], rng.random((50500, 1))), axis=1).astype(np.float32)
    b = glg.cluster_scan(big, np.full(50500, 72, np.uint32))       # terrain: tolerance 2 m -> one component
    assert len(b) == 0
    ok = glg.cluster_scan(big[:40000], np.full(40000, 72, np.uint32))
    assert len(ok) == 1 and int(ok.node_sizes[0]) == 40000 and int(ok.node_labels[0]) == 9
    # 5. more nodes than the caller allowed for: loud
    with pytest.raises(engine.SgprError):
        glg.cluster_scan(pts, lab, max_nodes=3)
    with pytest.raises(ValueError):
        glg.cluster_scan(pts, lab[:-1])


def test_scan_to_graph_feeds_the_scorer(tmp_path, go, ckpt_path):
    """End to end: scan -> graph JSON (reference layout) -> process_pair / eval_batch_pair of the scorer."""
    from sg_pr_amd import synth, gen_label_graph as glg, sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    paths = []
    for s in range(2):
        pts, lab = synth.labelled_scan(seed=10 + s, scale=0.4)
        pose = np.eye(4)[:3].reshape(-1).copy()
        pose[3], pose[11] = 30.0 * s, 1.0
        g = glg.scan_to_graph(pts, lab, pose=pose, with_edges=True)
        assert set(g) == {"nodes", "edges", "weights", "centers", "pose"} and len(g["pose"]) == 12
        want = go.gen_graphs(go.gen_labels(pts, lab), with_edges=False)
        assert g["nodes"] == want["nodes"]
        p = str(tmp_path / ("%06d.json" % s))
        with open(p, "w") as f:
            json.dump(g, f)
        paths.append(p)
    args = sgpr_args()
    args.model = ckpt_path
    trainer = sg_net.SGTrainer(args, False)
    pred, gt = trainer.eval_batch_pair([[paths[0], paths[0]], [paths[0], paths[1]]])
    assert pred.shape == (2,) and gt.tolist() == [1.0, 0.0] and pred[0] > 0.5
