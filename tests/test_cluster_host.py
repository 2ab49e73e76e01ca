"""The exact clustering reference (tests/cluster_ref.py) against the oracle, and the precondition of every scan generator
of tests/test_gpu_cluster.py: the property that makes its GPU test bite is proved here, on the CPU, so that no GPU case
is ever vacuous.  CPU only."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import cluster_ref as cr
from oracle import graph_oracle as go

THREE = [(cr.TRUNK, 0.2), (cr.FENCE, 0.5), (cr.VEGETATION, 2.0)]


def _min_separation(a, b, tol):
    """smallest distance between points of two DIFFERENT dumbbells"""
    ends = np.concatenate((a, b)).astype(np.float64)
    owner = np.concatenate((np.arange(len(a)), np.arange(len(b))))
    d, i = cKDTree(ends).query(ends, k=3)
    other = owner[i] != owner[:, None]
    return np.where(other, d, np.inf).min()


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_the_oracle_on_a_synthetic_scan(seed):
    from sg_pr_amd import synth
    pts, lab = synth.labelled_scan(seed, 0.5)
    ref = cr.cluster_ref(pts, lab)
    cl = go.gen_labels(pts, lab)
    want = go.gen_graphs(cl, with_edges=False)
    assert ref["node_labels"].tolist() == want["nodes"] and len(want["nodes"]) >= 20
    inst = cl[:, 5].astype(int)
    node_inst = [i for i in np.unique(inst) if int(cl[inst == i][0, 4]) not in (9, 10)]
    assert ref["node_sizes"].tolist() == [int((inst == i).sum()) for i in node_inst]
    # the per-point partition: the rows of every oracle cluster are the points the reference gives that node
    for k, i in enumerate(node_inst):
        mine = pts[ref["point_node"] == k].astype(np.float64)
        theirs = cl[inst == i][:, :4]
        assert np.array_equal(mine[np.lexsort(mine.T)], theirs[np.lexsort(theirs.T)])
    assert (ref["point_node"] >= 0).sum() == sum(int((inst == i).sum()) for i in node_inst)
    # centres: every coordinate is rounded to 2^-24 m by at most 2^-25 m and the mean of the roundings is no larger;
    # the conversion of the sum and the final scaling round twice more, the oracle's own float64 mean a little: 4 ulp
    oc = np.array(want["centers"])
    assert (np.abs(ref["centers"] - oc) <= 2.0 ** -25 + 4 * np.spacing(np.abs(oc))).all()


def test_reference_centre_bits_and_nonfinite_rule():
    pts = np.array([[0.3, -1.7, 2.0, 0], [0.1, 5.5, 2.0, 0]] * 11, dtype=np.float32)       # 22 points, one instance
    lab = np.full(22, 10 | (4 << 16), dtype=np.uint32)
    ref = cr.cluster_ref(pts, lab)
    s = sum(int(np.rint(np.float64(v) * 2 ** 24)) for v in pts[:, 0])
    assert ref["centers"][0, 0] == np.float64(s) * (1.0 / (16777216.0 * 22)) and ref["node_sizes"].tolist() == [22]
    pts[3, 1] = np.inf
    bad = cr.cluster_ref(pts, lab)
    assert np.isnan(bad["centers"][0, 1]) and np.array_equal(cr.bits(bad["centers"][0, [0, 2]]), cr.bits(ref["centers"][0, [0, 2]]))
    # Euclidean class: the non-finite point is dropped, the rest clusters as before
    e = np.zeros((60, 4), dtype=np.float32)
    e[7, 2] = np.nan
    got = cr.cluster_ref(e, np.full(60, cr.TRUNK, dtype=np.uint32))
    assert got["node_sizes"].tolist() == [59] and got["point_node"][7] == -1 and (np.delete(got["point_node"], 7) == 0).all()


def test_rounding_helper_and_fused_form():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    for v in rng.normal(size=200):
        assert cr.round_f32(Fraction(float(v))) == np.float32(v)
    one, eps = Fraction(1), Fraction(1, 2 ** 24)
    assert cr.round_f32(one + eps) == np.float32(1.0)                       # tie -> even
    assert cr.round_f32(one + 3 * eps) == np.float32(1.0 + 2.0 ** -22)      # tie -> even, upwards
    assert cr.round_f32(one + eps + Fraction(1, 2 ** 80)) == np.nextafter(np.float32(1), np.float32(2))
    # where the products are exact in float32 the fused form is the plain one
    a = rng.integers(-64, 64, size=(50, 3)).astype(np.float32) / 8
    assert np.array_equal(cr.f32_d2_fused(a, 0 * a), cr.f32_d2(a, 0 * a))


@pytest.mark.parametrize("raw,tol", THREE)
def test_threshold_scan_holds_every_rounding_group_and_every_cell_offset(raw, tol):
    """cases a and b"""
    pts, lab, a, b, a_first = cr.threshold_scan(tol, raw)
    g = cr.classify(a, b, tol)
    for name in ("equal", "reassoc", "fused", "fused_inner", "f64"):
        assert g[name].sum() >= 20, (name, int(g[name].sum()))
    assert not g["linked"][g["equal"]].any()                               # d2 == tol2: not linked
    assert 200 <= len(a) <= 600 and len(lab) <= 200000
    assert _min_separation(a, b, tol) >= 3 * tol
    # b - a lies on the sphere of radius tol within +-3e-7 plus the float32 rounding of b (the hand cases: exactly)
    r = np.linalg.norm(b.astype(np.float64) - a.astype(np.float64), axis=1)
    assert (np.abs(r / tol - 1) < 3e-7 + 2 * np.spacing(np.float32(np.abs(a).max())) / tol).all()
    assert (a < 0).any(axis=0).all() and (a > 0).any(axis=0).all()
    # the hand-made axis cases: spacing exactly tol is not a link, one float32 below it is
    ha, hb = cr.axis_cases(tol)
    hg = cr.f32_d2(ha, hb) < cr.f32_tol(tol)[1]
    assert hg.tolist() == [False, True] * 6
    assert np.array_equal(np.abs(hb - ha).max(axis=1), np.tile([np.float32(tol), np.nextafter(np.float32(tol), np.float32(0))], 6))
    # the index order: every point of the low end lies below every point of the high end
    half = (cr.min_size_of(raw) + 1) // 2
    low, high = np.where(a_first[:, None], a, b), np.where(a_first[:, None], b, a)
    where = {}
    for p, v in enumerate(map(tuple, pts[:, :3].tolist())):
        lo, hi = where.get(v, (p, p))
        where[v] = (min(lo, p), max(hi, p))
    assert all(where[tuple(l.tolist())][1] < where[tuple(h.tolist())][0] for l, h in zip(low, high))
    assert 0.3 < a_first.mean() < 0.7
    # case b: only the high end of a dumbbell can find its link, in the cell offset cell(low) - cell(high): all 26
    # neighbour offsets occur there among the LINKED dumbbells, each at least twice; cells 0 / -1 straddled on every axis
    off = cr.lookup_offsets(a, b, a_first, tol)[g["linked"]]
    assert np.abs(off).max() == 1
    seen = {}
    for o in map(tuple, off.tolist()):
        seen[o] = seen.get(o, 0) + 1
    seen.pop((0, 0, 0), None)
    assert len(seen) == 26 and min(seen.values()) >= 2, seen
    ca, cb = cr.cell_coord(a, tol)[g["linked"]], cr.cell_coord(b, tol)[g["linked"]]
    for ax in range(3):
        assert ((np.minimum(ca[:, ax], cb[:, ax]) == -1) & (np.maximum(ca[:, ax], cb[:, ax]) == 0)).any()
    # the reference agrees with the classification: one node per linked dumbbell, of 2 * ceil(min / 2) points
    ref = cr.cluster_ref(pts, lab)
    assert ref["node_sizes"].tolist() == [2 * half] * int(g["linked"].sum())
    assert (ref["point_node"] >= 0).sum() == 2 * half * g["linked"].sum()


def test_a_missed_neighbour_cell_loses_nodes_of_the_threshold_scan():
    """The kernel's pair enumeration on the host (cluster_ref.emulate_nodes): complete, it is the reference's partition;
    with any ONE of the 26 neighbour offsets dropped from the lookup, exactly the dumbbells linked through that offset stop
    being nodes.  (Trunk scan: the other two differ in tolerance only.)"""
    pts, lab, a, b, a_first = cr.threshold_scan(0.2, cr.TRUNK)
    ref = cr.cluster_ref(pts, lab)
    first = [int(np.flatnonzero(ref["point_node"] == k)[0]) for k in range(len(ref["node_sizes"]))]
    pairs = cr.emulation_pairs(pts, 0.2)
    full = cr.emulate_nodes(pts, 0.2, 50, pairs=pairs)
    assert full == sorted(zip(ref["node_sizes"].tolist(), first))
    linked = cr.f32_d2(a, b) < cr.f32_tol(0.2)[1]
    off = cr.lookup_offsets(a, b, a_first, 0.2)
    for d in [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]:
        lost = int((linked & (off == np.array(d)).all(axis=1)).sum())
        assert lost >= 2 and len(cr.emulate_nodes(pts, 0.2, 50, dropped=[d], pairs=pairs)) == len(full) - lost, d
    # a whole slab, as in a neighbour loop that starts at dz = 0
    slab = [(x, y, -1) for x in (-1, 0, 1) for y in (-1, 0, 1)]
    assert len(cr.emulate_nodes(pts, 0.2, 50, dropped=slab, pairs=pairs)) == len(full) - int((linked & (off[:, 2] == -1)).sum()) < len(full) - 10


def test_far_scan_has_linked_and_unlinked_dumbbells_on_the_4mm_grid():
    pts, lab, parts = cr.far_scan()
    ref = cr.cluster_ref(pts, lab)
    assert np.abs(pts[:, :2]).min() > 39000 and np.abs(pts[:, :3]).max() < 41000
    assert np.spacing(np.float32(40000.0)) == 2.0 ** -8
    want = []
    for raw, tol, a, b, a_first in parts:
        linked = cr.f32_d2(a, b) < cr.f32_tol(tol)[1]
        assert 4 <= linked.sum() <= len(a) - 4
        assert _min_separation(a, b, tol) >= 3 * tol
        assert np.abs(cr.cell_coord(a, tol)).max() < 2 ** 18                # no key wrap here: case c is the wrap
        want.append((go.NODE_MAP[go.LEARNING_MAP[raw]], int(linked.sum())))
    got = sorted((int(l), int((ref["node_labels"] == l).sum())) for l in np.unique(ref["node_labels"]))
    assert got == sorted(want)


def test_alias_scan_shares_one_19_bit_key():
    pts, lab, info = cr.alias_scan()
    ia, ib, ic = (int(cr.cell_coord(info[k], 0.2)) for k in ("ax", "bx", "cx"))
    assert ib - ia == 2 ** 19 and ic - ia in (0, 1)
    assert (cr.cell_coord(pts[:, 1:3], 0.2) == 0).all()
    assert cr.cell_key(16, (ia, 0, 0)) == cr.cell_key(16, (ib, 0, 0))
    assert np.abs(pts[:, :3]).max() < 110000
    ref = cr.cluster_ref(pts, lab)
    assert ref["node_sizes"].tolist() == [115, 70] and ref["node_labels"].tolist() == [8, 8]
    x = pts[:, 0]
    assert (ref["point_node"][x < 0] == 0).all() and (ref["point_node"][x > 0] == 1).all()
    assert np.array_equal(np.unique(x), np.sort([info["ax"], info["cx"], info["bx"]]))


def test_size_scans_sit_on_every_size_rule():
    pts, lab = cr.size_scan_euclidean()
    assert len(lab) <= 200000
    ref = cr.cluster_ref(pts, lab)
    want_l, want_s = [], []
    for c in sorted(cr.EUCLID_RAW):
        mn = go.cluster_params(c)[1]
        sizes = [mn + 1, mn]                                               # min_size - 1 is not a node
        if c == 17:
            sizes = [50000] + sizes                                        # 50 001 is not a node
        want_l += [go.NODE_MAP[c]] * len(sizes)
        want_s += sizes
    assert ref["node_labels"].tolist() == want_l and ref["node_sizes"].tolist() == want_s
    sem, _ = cr.remap(lab)
    for c in sorted(cr.EUCLID_RAW):                                        # the lattices and blobs are what they claim
        mn = go.cluster_params(c)[1]
        assert (sem == c).sum() == 3 * mn + (100001 if c == 17 else 0)
    pts, lab = cr.size_scan_instances()
    ref = cr.cluster_ref(pts, lab)
    # class 1: ids 2 (21 points) and 3 (50 001); id 4 (20 points) is dropped.  trunk 50 (49 dropped), fence 100
    assert ref["node_labels"].tolist() == [0, 0, 6, 8] and ref["node_sizes"].tolist() == [21, 50001, 100, 50]
    assert len(lab) <= 200000


def test_label_scans_cover_the_whole_table():
    assert cr.N_RAW == 359
    for inst in (0, 7):
        pts, lab = cr.every_label_scan(inst)
        assert np.array_equal(np.unique(lab & 0xFFFF), np.arange(359)) and (np.bincount(lab & 0xFFFF) == 320).all()
        assert (lab >> 16 == inst).all() and len(lab) <= 200000
        ref = cr.cluster_ref(pts, lab)
        per_class = {c: sum(1 for r, v in go.LEARNING_MAP.items() if v == c) for c in go.NODE_MAP}
        if inst == 0:                                                      # Euclidean: one node of 320 per raw id
            want = [(go.NODE_MAP[c], 320) for c in sorted(go.NODE_MAP) for _ in range(per_class[c])]
        else:                                                              # one instance per class: the raw ids merge
            want = [(go.NODE_MAP[c], 320 * per_class[c]) for c in sorted(go.NODE_MAP)]
        assert list(zip(ref["node_labels"].tolist(), ref["node_sizes"].tolist())) == want
    pts, lab = cr.mixed_mode_scan()
    ref = cr.cluster_ref(pts, lab)
    # class 1: ids 7 (30) and 9 (15 + 15 under raw 10 and 252); class 4: id 7; class 5: ids 0 (two blobs 50 m apart, one
    # node), 5 and 65535; trunk: one Euclidean node; pole: two
    assert ref["node_labels"].tolist() == [0, 0, 1, 2, 2, 2, 8, 10, 10]
    assert ref["node_sizes"].tolist() == [30, 30, 35, 60, 40, 25, 60, 101, 100]
    zero = pts[lab == 13][:, 0]
    assert zero.max() - zero.min() > 49


def test_order_scan_has_known_ties():
    pts, lab, blob = cr.order_scan()
    ref = cr.cluster_ref(pts, lab)
    assert blob[:5].tolist() == cr.EQUAL_ORDER
    assert ref["node_labels"].tolist() == [0] * 4 + [6] * 8
    assert ref["node_sizes"].tolist() == [90, 70, 50, 30, 160, 140, 120, 120, 120, 120, 120, 105]
    # the five equal clusters come out in the order of their lowest point indices
    assert [int(blob[np.flatnonzero(ref["point_node"] == 6 + k)[0]]) for k in range(5)] == cr.EQUAL_ORDER
    rev = cr.cluster_ref(pts[::-1], lab[::-1])
    assert cr.node_multiset(rev) == cr.node_multiset(ref)
    assert [int(blob[::-1][np.flatnonzero(rev["point_node"] == 6 + k)[0]]) for k in range(5)] != cr.EQUAL_ORDER


def test_chain_is_one_component_and_the_gap_cuts_it():
    xyz, split = cr.chain_scan()
    assert split is None and len(xyz) == 20000
    step = np.sqrt(cr.f32_d2(xyz[1:], xyz[:-1]).astype(np.float64))
    assert (cr.f32_d2(xyz[1:], xyz[:-1]) < cr.f32_tol(0.2)[1]).all() and step.min() > 0.18
    ref = cr.cluster_ref(*cr.chain_points(xyz, np.arange(20000)))
    assert ref["node_sizes"].tolist() == [20000] and (ref["point_node"] == 0).all()
    # a chain, not a sheet: every point has at most two neighbours in range
    pairs = cKDTree(xyz.astype(np.float64)).query_pairs(0.2001, output_type="ndarray")
    pairs = pairs[cr.f32_d2(xyz[pairs[:, 0]], xyz[pairs[:, 1]]) < cr.f32_tol(0.2)[1]]
    assert len(pairs) == 19999 and np.bincount(pairs.ravel()).max() == 2
    # rows meet in the neighbour lookups: thousands of pairs of points of two DIFFERENT rows (connectors left out) lie in
    # neighbouring cells, where the lookup finds them, and are out of range, so only the distance test keeps rows apart
    half = np.round(xyz[:, 1] / 0.19).astype(int)
    near = cKDTree(xyz.astype(np.float64)).query_pairs(0.45, output_type="ndarray")
    i, j = near[:, 0], near[:, 1]
    across = (half[i] % 2 == 0) & (half[j] % 2 == 0) & (half[i] != half[j])
    seen = np.abs(cr.cell_coord(xyz[i], 0.2) - cr.cell_coord(xyz[j], 0.2)).max(axis=1) <= 1
    assert (across & seen).sum() > 5000
    assert not (cr.f32_d2(xyz[i], xyz[j])[across] < cr.f32_tol(0.2)[1]).any()
    gx, split = cr.chain_scan(gap_row=50)
    assert split == 50 * 201 + 1
    assert gx[split, 0] - gx[split - 1, 0] == np.float32(0.2) and cr.f32_d2(gx[split], gx[split - 1]) == cr.f32_tol(0.2)[1]
    ref = cr.cluster_ref(*cr.chain_points(gx, np.arange(20000)))
    assert ref["node_sizes"].tolist() == sorted([split, 20000 - split], reverse=True)


@pytest.mark.parametrize("isolated", [411, 412, 413, 511, 512, 513, 3996, 4096])
def test_occupancy_scan_fills_one_cell_per_point(isolated):
    pts, lab = cr.occupancy_scan(isolated)
    assert len(lab) == isolated + 100
    cells = np.unique(cr.cell_coord(pts[:, :3], 0.2), axis=0)
    assert len(cells) == isolated + 4
    ref = cr.cluster_ref(pts, lab)
    assert ref["node_sizes"].tolist() == [50] and (ref["point_node"] >= 0).sum() == 50
    # the scan sizes 511 / 512 / 513 / 4096 are where the table size steps
    assert [cr.table_slots(p) for p in (511, 512, 513, 4096, 4097)] == [1024, 1024, 2048, 8192, 16384]


def test_instance_scans_sit_on_the_candidate_limit():
    pts, lab = cr.instance_scan(cr.MAX_CAND)
    assert len(lab) == 8192 * 21 <= 200000
    import time
    t = time.perf_counter()
    ref = cr.cluster_ref(pts, lab)
    # vectorised: 8 192 instances take about 0.1 s; one flatnonzero per instance over 172 032 points would take minutes
    assert time.perf_counter() - t < 10.0
    assert ref["node_sizes"].tolist() == [21] * 8192 and (ref["node_labels"] == 0).all()
    first = np.unique(ref["point_node"], return_index=True)[1]
    assert ((lab[first] >> 16) == np.arange(1, 8193)).all()                # nodes in instance id order
    pts, lab = cr.instance_scan(cr.MAX_CAND + 1)
    assert len(np.unique(lab)) == 8193 <= 32768 and len(lab) <= 200000


def test_poisoned_scans_change_what_they_should():
    pts, lab, cases = cr.poisoned_scans()
    clean = cr.cluster_ref(pts, lab)
    for name, (bad, plan) in cases.items():
        ref = cr.cluster_ref(bad, lab)
        hit = np.array([p for p, _, _ in plan])
        assert ref["node_labels"].tolist() == clean["node_labels"].tolist(), name
        if name == "remission":
            assert all(np.array_equal(ref[k], clean[k]) for k in ("node_sizes", "point_node"))
            assert np.array_equal(cr.bits(ref["centers"]), cr.bits(clean["centers"]))
        elif name == "euclid_road":
            assert (ref["point_node"][hit] == -1).all() and (clean["point_node"][hit] >= 0).sum() >= 6
            lost = np.bincount(clean["point_node"][hit][clean["point_node"][hit] >= 0], minlength=len(clean["node_sizes"]))
            assert np.array_equal(ref["node_sizes"], clean["node_sizes"] - lost)
            rest = np.setdiff1d(np.arange(len(lab)), hit)
            assert np.array_equal(ref["point_node"][rest], clean["point_node"][rest])
            assert np.isfinite(ref["centers"]).all()
        else:
            (p, col, _), = plan
            node = clean["point_node"][p]
            assert node >= 0 and np.array_equal(ref["point_node"], clean["point_node"])
            assert np.array_equal(ref["node_sizes"], clean["node_sizes"])
            nan = np.isnan(ref["centers"])
            assert nan.sum() == 1 and nan[node, col]
            assert np.array_equal(cr.bits(ref["centers"])[~nan], cr.bits(clean["centers"])[~nan])


def test_edge_reference_on_dyadic_and_general_coordinates():
    for swap in (False, True):
        pts, pn, c = cr.dyadic_edge_case(swap)
        near, dis = cr.edges_ref(pts, pn, c)
        assert near[0, 1] == 0 and near[1, 0] == 2                         # the lower scan index among equals
        assert dis[0, 1] == (np.sqrt(8.0) if swap else 2.0) and dis[2, 3] == 5.0 and dis[3, 2] == 5.0
        assert (np.diag(dis) == 0).all()
    # a node without points, and a NaN centre
    pn2 = pn.copy()
    pn2[pn2 == 1] = -1
    near, dis = cr.edges_ref(pts, pn2, c)
    off = ~np.eye(4, dtype=bool)
    assert np.isnan(dis[1][off[1]]).all() and np.isnan(dis[:, 1][off[1]]).all() and dis[2, 3] == 5.0 and dis[0, 2] > 0
    c2 = c.copy()
    c2[0, 1] = np.nan
    assert np.isnan(cr.edges_ref(pts, pn, c2)[1][0, 1:]).all()
    # against the oracle's float64 form on a synthetic scan: same edges, distances within 2 ulp
    from sg_pr_amd import synth
    p, l = synth.labelled_scan(4, 0.3)
    ref = cr.cluster_ref(p, l)
    _, dis = cr.edges_ref(p, ref["point_node"], ref["centers"])
    want = go.gen_graphs(go.gen_labels(p, l))
    n = len(ref["node_labels"])
    edges = [[i, j] for i in range(n - 1) for j in range(i + 1, n) if dis[i, j] <= 5.0]
    assert edges == want["edges"] and len(edges) > 0
    w = np.array([1 - dis[i, j] / 5.0 for i, j in edges])
    assert np.abs(w - np.array(want["weights"])).max() < 1e-9
    assert cr.sqrt_f64(cr.Fraction(2)) == np.sqrt(2.0) and cr.sqrt_f64(cr.Fraction(25)) == 5.0
