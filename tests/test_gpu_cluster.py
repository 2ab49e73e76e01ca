"""sgpr_cluster_scan / sgpr_graph_edges (sg_pr_amd/csrc/sgpr_cluster.hip) at the boundaries of their rules, against the
exact host reference tests/cluster_ref.py.  Every comparison is exact - integer arrays with array_equal, centres by
bit pattern - except the one 2-ulp bound on edge distances of general coordinates (derived at its test).  The scans come
from seeded generators in cluster_ref.py; tests/test_cluster_host.py proves on the CPU that each of them holds the cases
it is meant to hold (the rounding groups, the 26 cell offsets, the key alias, the exact sizes).  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import cluster_ref as cr

pytestmark = pytest.mark.gpu


def _run(pts, lab, max_nodes=1024):
    from sg_pr_amd import gen_label_graph as glg
    sc = glg.cluster_scan(pts, lab, max_nodes=max_nodes)
    return sc, {"node_labels": sc.node_labels.cpu().numpy(), "node_sizes": sc.node_sizes.cpu().numpy(),
                "point_node": sc.point_node.cpu().numpy(), "centers": sc.centers.cpu().numpy()}


def _same(got, want, what=""):
    for k in ("node_labels", "node_sizes", "point_node"):
        assert got[k].dtype == np.int32
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))
    assert got["centers"].dtype == np.float64 and got["centers"].shape == want["centers"].shape
    np.testing.assert_array_equal(cr.bits(got["centers"]), cr.bits(want["centers"]), err_msg="%s centre bits" % what)


def _check(pts, lab, max_nodes=1024, what=""):
    assert len(lab) <= 200000
    sc, got = _run(pts, lab, max_nodes)
    want = cr.cluster_ref(pts, lab)
    _same(got, want, what)
    return sc, got, want


@pytest.mark.parametrize("raw,tol", [(cr.TRUNK, 0.2), (cr.FENCE, 0.5), (cr.VEGETATION, 2.0)])
def test_distance_threshold_rounding_and_cell_straddling(raw, tol):
    """cases a + b: dumbbells whose ends are one tolerance apart to within 3e-7 - at least 20 each with d2 == tol2, with a
    decision that flips under re-association, under contraction and in float64 - over all 26 neighbour-cell offsets and
    across cells 0 / -1, plus the axis-aligned spacings tol and nextafter(tol, 0).  A dumbbell is a node iff its ends link,
    and its index order lets only one end find the link: all 26 lookup offsets occur (tests/test_cluster_host.py)."""
    pts, lab, a, b, _ = cr.threshold_scan(tol, raw)
    _, got, _ = _check(pts, lab)
    linked = cr.f32_d2(a, b) < cr.f32_tol(tol)[1]
    assert len(got["node_labels"]) == linked.sum()
    # which dumbbells became nodes: the ones the kernel's formula links, one by one
    node_at = {}
    for p in np.flatnonzero(got["point_node"] >= 0):
        node_at.setdefault(tuple(pts[p, :3].tolist()), set()).add(int(got["point_node"][p]))
    for k in range(len(a)):
        ends = [node_at.get(tuple(v.tolist())) for v in (a[k], b[k])]
        assert (ends[0] is not None and ends[0] == ends[1] and len(ends[0]) == 1) if linked[k] else ends == [None, None], k


def test_dumbbells_40_km_out():
    """case b: float32 is spaced 2^-8 m here; linked and unlinked dumbbells of all three tolerances"""
    pts, lab, _ = cr.far_scan()
    _check(pts, lab)


def test_two_clusters_on_one_cell_key_stay_apart():
    """case c: cell indices 2^19 apart share the 19-bit key; only the distance test separates them"""
    pts, lab, _ = cr.alias_scan()
    _, got, _ = _check(pts, lab)
    assert got["node_sizes"].tolist() == [115, 70]


def test_size_rules_on_their_boundaries():
    """case d: min_size - 1 / min_size / min_size + 1 for every Euclidean class, lattices of 50 000 and 50 001 points,
    instance groups of 20, 21 and 50 001 points"""
    _, got, _ = _check(*cr.size_scan_euclidean(), what="euclidean")
    assert 50000 in got["node_sizes"] and 50001 not in got["node_sizes"]
    _, got, _ = _check(*cr.size_scan_instances(), what="instances")
    assert got["node_sizes"].tolist() == [21, 50001, 100, 50]


@pytest.mark.parametrize("inst", [0, 7])
def test_every_raw_label(inst):
    """case e: raw ids 0 .. 358, Euclidean (instance id 0) and instance-grouped (7)"""
    _, got, _ = _check(*cr.every_label_scan(inst))
    from oracle import graph_oracle as go
    assert len(got["node_labels"]) == (sum(v in go.NODE_MAP for v in go.LEARNING_MAP.values()) if inst == 0 else 12) >= 12


def test_modes_of_one_class_side_by_side():
    """case e: id-0 points of an instance-labelled class are one group however far apart; one id under two classes is two
    nodes; raw 10 and 252 with one id are one node; a class with id 0 only is clustered by distance"""
    _, got, _ = _check(*cr.mixed_mode_scan())
    assert got["node_sizes"].tolist() == [30, 30, 35, 60, 40, 25, 60, 101, 100]


def test_node_order_under_point_permutations():
    """case f: equal sizes rank by lowest point index, sizes descend, instance ids ascend - for three point orders"""
    pts, lab, blob = cr.order_scan()
    rng = np.random.default_rng(1)
    keys = []
    for name, perm in (("identity", np.arange(len(lab))), ("reversed", np.arange(len(lab))[::-1]), ("random", rng.permutation(len(lab)))):
        p, l = np.ascontiguousarray(pts[perm]), np.ascontiguousarray(lab[perm])
        _, got, _ = _check(p, l, what=name)
        keys.append(cr.node_multiset(got))
        if name == "identity":
            assert [int(blob[np.flatnonzero(got["point_node"] == 6 + k)[0]]) for k in range(5)] == cr.EQUAL_ORDER
    assert keys[0] == keys[1] == keys[2]


@pytest.mark.parametrize("gap_row", [None, 50])
def test_union_find_on_a_20000_point_chain(gap_row):
    """case g: one component 20 000 links deep, in ascending, descending and random index order; with one step of exactly
    0.2f, two components"""
    xyz, split = cr.chain_scan(gap_row=gap_row)
    rng = np.random.default_rng(2)
    keys = []
    for name, order in (("ascending", np.arange(20000)), ("descending", np.arange(20000)[::-1]), ("random", rng.permutation(20000))):
        _, got, _ = _check(*cr.chain_points(xyz, order), what=name)
        if gap_row is None:
            assert got["node_sizes"].tolist() == [20000] and (got["point_node"] == 0).all()
        else:
            assert sorted(got["node_sizes"].tolist()) == sorted([split, 20000 - split])
            first = got["point_node"][np.argsort(order)][:split]                 # back in chain order
            assert (first == first[0]).all() and (got["point_node"][np.argsort(order)][split:] == 1 - first[0]).all()
        keys.append(cr.node_multiset(got))
    assert keys[0] == keys[1] == keys[2]


@pytest.mark.parametrize("isolated", [411, 412, 413, 511, 512, 513, 3996, 4096])
def test_cell_table_at_its_highest_load(isolated):
    """case h: one point per cell around the scan sizes (511, 512 | 513, 4096) at which the table changes size, counted
    with the 100 points of the two dumbbells and without them"""
    pts, lab = cr.occupancy_scan(isolated)
    _, got, _ = _check(pts, lab)
    assert got["node_sizes"].tolist() == [50] and (got["point_node"] >= 0).sum() == 50


def test_candidate_limit():
    """case i: 8 192 instance groups are all nodes, in id order; 8 193 are refused by name"""
    from sg_pr_amd import engine, gen_label_graph as glg
    pts, lab = cr.instance_scan(cr.MAX_CAND)
    _, got, _ = _check(pts, lab, max_nodes=cr.MAX_CAND)
    assert len(got["node_sizes"]) == 8192
    pts, lab = cr.instance_scan(cr.MAX_CAND + 1)
    with pytest.raises(engine.SgprError, match="> 8192"):
        glg.cluster_scan(pts, lab, max_nodes=cr.MAX_CAND)


@pytest.fixture(scope="module")
def poisoned():
    pts, lab, cases = cr.poisoned_scans()
    return pts, lab, cases, cr.cluster_ref(pts, lab)


def _edge_check(sc, got, want_dis):
    """device edge distances against the exact ones: NaN where the reference is NaN, within 2 ulp elsewhere"""
    from sg_pr_amd import engine
    d = engine.graph_edges(sc.points, sc.point_node, sc.centers).cpu().numpy()
    nan = np.isnan(want_dis)
    np.testing.assert_array_equal(np.isnan(d), nan)
    assert (cr.ulp_distance(d[~nan], want_dis[~nan]) <= 2).all()
    return d


@pytest.mark.parametrize("name", ["car_nan_x", "truck_inf_z", "euclid_road", "remission"])
def test_non_finite_coordinates(poisoned, name):
    """case j: an axis of a centre is NaN iff a point of the cluster is non-finite on it, the other axes keep their bits;
    under Euclidean clustering and in road such a point only drops out; remission is never read.  Edges: the NaN node's
    row and column are NaN (no edge), every other distance is the reference's."""
    from sg_pr_amd import gen_label_graph as glg
    pts, lab, cases, clean = poisoned
    bad, plan = cases[name]
    sc, got, want = _check(bad, lab, what=name)
    np.testing.assert_array_equal(got["node_labels"], clean["node_labels"])
    nan = np.isnan(got["centers"])
    if name == "remission":
        _same(got, clean, "remission")
    elif name == "euclid_road":
        assert not nan.any() and (got["point_node"][[p for p, _, _ in plan]] == -1).all()
    else:
        (p, col, _), = plan
        node = clean["point_node"][p]
        assert nan.sum() == 1 and nan[node, col]
        np.testing.assert_array_equal(got["node_sizes"], clean["node_sizes"])
        np.testing.assert_array_equal(cr.bits(got["centers"])[~nan], cr.bits(clean["centers"])[~nan])
    _, want_dis = cr.edges_ref(bad, want["point_node"], want["centers"])
    d = _edge_check(sc, got, want_dis)
    g = glg.gen_graphs(sc, with_edges=True)
    n = len(got["node_labels"])
    assert g["edges"] == [[i, j] for i in range(n - 1) for j in range(i + 1, n) if want_dis[i, j] <= 5.0]
    if nan.any():
        node = int(np.flatnonzero(nan.any(axis=1))[0])
        off = np.arange(n) != node
        assert np.isnan(d[node, off]).all() and np.isnan(d[off, node]).all() and d[node, node] == 0
        assert all(node not in e for e in g["edges"]) and len(g["edges"]) > 0


def _edges(pts, point_node, centers):
    from sg_pr_amd import engine
    return engine.graph_edges(torch.from_numpy(pts).cuda(), torch.from_numpy(point_node).cuda(),
                              torch.from_numpy(centers).cuda()).cpu().numpy()


def test_edges_on_dyadic_coordinates_are_exact():
    """case k: multiples of 1/8 m, so every product and sum is exact in float64 and contraction cannot matter: the lower
    scan index wins among equidistant points, a distance of exactly 5.0 is an edge of weight 0.0, nextafter(5, 6) is none;
    n = 1 and n = 2; a node no point carries gives NaN in its row and column"""
    from sg_pr_amd import gen_label_graph as glg
    for swap in (False, True):
        pts, pn, c = cr.dyadic_edge_case(swap)
        _, want = cr.edges_ref(pts, pn, c)
        got = _edges(pts, pn, c)
        np.testing.assert_array_equal(cr.bits(got), cr.bits(want))
        assert got[0, 1] == (np.sqrt(8.0) if swap else 2.0) and got[2, 3] == 5.0
    sc = glg.ScanClusters(torch.from_numpy(pts).cuda(), None, torch.from_numpy(c).cuda(), torch.zeros(4, dtype=torch.int32),
                          torch.ones(4, dtype=torch.int32), torch.from_numpy(pn).cuda())
    g = glg.gen_graphs(sc)
    assert [2, 3] in g["edges"] and g["weights"][g["edges"].index([2, 3])] == 0.0
    # one float32 past 5.0: no edge
    five = np.nextafter(np.float32(5), np.float32(6))
    p2 = np.array([(0, 0, 0), (five, 0, 0)], dtype=np.float32)
    pn2, c2 = np.array([0, 1], dtype=np.int32), p2.astype(np.float64)
    got = _edges(p2, pn2, c2)                                                      # n = 2
    np.testing.assert_array_equal(cr.bits(got), cr.bits(cr.edges_ref(p2, pn2, c2)[1]))
    assert got[0, 1] == np.float64(five) > 5.0
    sc2 = glg.ScanClusters(torch.from_numpy(p2).cuda(), None, torch.from_numpy(c2).cuda(), torch.zeros(2, dtype=torch.int32),
                           torch.ones(2, dtype=torch.int32), torch.from_numpy(pn2).cuda())
    assert glg.gen_graphs(sc2)["edges"] == []
    got = _edges(p2, np.zeros(2, dtype=np.int32), c2[:1])                          # n = 1
    assert got.shape == (1, 1) and got[0, 0] == 0.0
    # node 1 without points
    pts, pn, c = cr.dyadic_edge_case()
    pn = np.where(pn == 1, -1, pn).astype(np.int32)
    _, want = cr.edges_ref(pts, pn, c)
    got = _edges(pts, pn, c)
    np.testing.assert_array_equal(cr.bits(got), cr.bits(want))
    off = np.arange(4) != 1
    assert np.isnan(got[1, off]).all() and np.isnan(got[off, 1]).all() and got[2, 3] == 5.0


def test_edges_on_general_coordinates_within_2_ulp():
    """case k: the device may fuse dx*dx + dy*dy, which saves roundings but adds none, then takes one correctly rounded
    sqrt.  Unfused, three products and two sums round under the root: at most 2.5 ulp on the sum of squares, which the
    root halves to 1.25 ulp; with the root's own half ulp about 1.75 ulp on the distance: 2 ulp, rounded up."""
    from sg_pr_amd import synth
    pts, lab = synth.labelled_scan(4, 0.3)
    sc, got, want = _check(pts, lab)
    _, want_dis = cr.edges_ref(pts, want["point_node"], want["centers"])
    assert np.isfinite(want_dis).all() and len(want_dis) >= 15
    _edge_check(sc, got, want_dis)
