"""Exact host reference of the scan -> graph front end (include/sgpr.h: sgpr_cluster_scan, sgpr_graph_edges) and the
seeded scan generators of tests/test_gpu_cluster.py.  TEST INFRASTRUCTURE ONLY.

`cluster_ref(points, label)` returns what sgpr_cluster_scan returns, bit for bit:

  * the partition is the oracle's (oracle/graph_oracle.py: LEARNING_MAP, cluster_params, euclidean_clusters), grouped
    with np.unique instead of one flatnonzero per instance; nodes in the documented order - class ascending, then
    instance id ascending, or size descending with the lowest point index first among equal sizes;
  * centres carry the kernel's bits: s = sum over the cluster of int(rint(float64(x) * 2^24)) as an int64 (x * 2^24 is
    exact in float64; rint and the device's llrint both round half to even), centre = float64(s) * (1 / (2^24 * n));
  * non-finite coordinates: an axis of a centre is NaN iff some point of the cluster has a NaN / inf on that axis, the
    other axes sum every point.  Only an instance group can hold such a point.  Under Euclidean clustering every
    comparison with a non-finite coordinate is false, so such a point is a cluster of one, below every minimum size,
    with point_node = -1: the reference REMOVES these points before it calls the oracle (scipy's cKDTree refuses them:
    "ValueError: data must be finite").

`edges_ref` is gen_graphs' edge rule in exact arithmetic; see its docstring.

The `*_scan` functions build the scans of the GPU tests; `tests/test_cluster_host.py` proves, on the CPU, the property
that makes each of them bite (`f32_*` and `cell_*` restate the kernel's float32 formulas for that purpose)."""
import decimal
from fractions import Fraction

import numpy as np

from oracle import graph_oracle as go

FIX = 16777216.0                 # 2^24: the kernel's fixed-point scale
MAX_CAND = 8192                  # clusters that may qualify in one scan (sgpr.h)
# raw id -> (class, tolerance, minimum size) of the three Euclidean tolerances the boundary cases use
TRUNK, FENCE, VEGETATION = 71, 51, 70
EUCLID_RAW = {1: 10, 4: 18, 5: 13, 11: 48, 12: 49, 13: 50, 14: 51, 15: 70, 16: 71, 17: 72, 18: 80, 19: 81}


def remap(label):
    """raw label words -> (training class, instance id); ids past the reference's table are class 0, as on the device"""
    label = np.asarray(label).reshape(-1).astype(np.uint32)
    lut = go.remap_lut()
    raw = (label & 0xFFFF).astype(np.int64)
    sem = np.where(raw < len(lut), lut[np.minimum(raw, len(lut) - 1)], 0).astype(np.int64)
    return sem, (label >> 16).astype(np.int64)


def partition(points, label):
    """-> (node_labels [n], node_sizes [n], point_node [P]) of gen_labels + the node half of gen_graphs."""
    points = np.asarray(points, dtype=np.float32)
    sem, inst = remap(label)
    point_node = np.full(len(sem), -1, dtype=np.int32)
    labels, sizes = [], []
    for c in sorted(go.NODE_MAP):                        # the clustered classes are exactly the node classes
        idx = np.flatnonzero(sem == c)
        if idx.size == 0:
            continue
        base = len(labels)
        if (inst[idx] != 0).any():                       # instance labels present: group by id, ids ascending
            ids, inv, cnt = np.unique(inst[idx], return_inverse=True, return_counts=True)
            keep = cnt > 20
            rank = np.cumsum(keep) - 1
            point_node[idx] = np.where(keep[inv], base + rank[inv], -1)
            kept = cnt[keep].tolist()
        else:
            # a point with a non-finite coordinate is in range of nothing: a singleton below every minimum size.
            # cKDTree refuses non-finite data, so these points are removed here and keep point_node = -1
            idx = idx[np.isfinite(points[idx, :3]).all(axis=1)]
            tol, mn = go.cluster_params(c)
            groups = go.euclidean_clusters(points[idx, :3], tol, mn)
            for k, g in enumerate(groups):
                point_node[idx[g]] = base + k
            kept = [len(g) for g in groups]
        labels += [go.NODE_MAP[c]] * len(kept)
        sizes += kept
    return np.array(labels, dtype=np.int32), np.array(sizes, dtype=np.int32), point_node


def centres(points, point_node, sizes):
    """the kernel's centres, bit for bit (see the module docstring) -> float64 [n, 3]"""
    xyz = np.asarray(points, dtype=np.float32)[:, :3].astype(np.float64)
    n = len(sizes)
    on = point_node >= 0
    fin = np.isfinite(xyz)
    q = np.zeros(xyz.shape, dtype=np.int64)
    q[fin] = np.rint(xyz[fin] * FIX).astype(np.int64)
    s = np.zeros((n, 3), dtype=np.int64)
    bad = np.zeros((n, 3), dtype=bool)
    np.add.at(s, point_node[on], q[on])
    np.logical_or.at(bad, point_node[on], ~fin[on])
    inv = 1.0 / (FIX * np.asarray(sizes, dtype=np.float64))
    out = s.astype(np.float64) * inv[:, None]
    out[bad] = np.nan
    return out


def cluster_ref(points, label):
    """-> dict(node_labels i32 [n], node_sizes i32 [n], point_node i32 [P], centers f64 [n,3]) = sgpr_cluster_scan"""
    labels, sizes, point_node = partition(points, label)
    return {"node_labels": labels, "node_sizes": sizes, "point_node": point_node,
            "centers": centres(points, point_node, sizes)}


def bits(a):
    """float64 array -> its bit patterns (NaN compares by payload, -0.0 differs from +0.0)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def node_multiset(r):
    """sorted (label, size, centre bits): what must not depend on the point order"""
    return sorted(zip(r["node_labels"].tolist(), r["node_sizes"].tolist(), map(tuple, bits(r["centers"]).tolist())))


# ---- edges --------------------------------------------------------------------------------------------------------

def sqrt_f64(fr):
    """the square root of a non-negative Fraction, rounded once to float64 (50 digits, then the conversion's rounding)"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float((decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)).sqrt())


def _frac3(v):
    return [Fraction(float(x)) for x in v]


def edges_ref(points, point_node, centers):
    """gen_graphs' edge rule (gen_label_graph.py:367-385) in exact arithmetic -> (near int [n,n], min_dis f64 [n,n]).

    For i != j, near[i, j] is the point of node i nearest to the midpoint of the two centres (the float64 value
    (c_i + c_j) * 0.5 the oracle and the kernel both form), FIRST IN SCAN ORDER AMONG EQUALS, and min_dis[i, j] is the
    exact distance between near[i, j] and near[j, i], rounded once to float64.  The choice compares SQUARED distances,
    exactly (Fractions), as the kernel compares squared distances: np.argmin over square-rooted distances, the
    oracle's form, can differ where two squared distances differ yet round to one root, and only there.  A float64
    pass first narrows the choice to the points within 1e-12 (relative) of the smallest squared distance - its own
    error is below 1e-15 - and the exact comparison runs among those.
    near is -1 where the midpoint is NaN or no point carries node i; min_dis is NaN where either index is -1, 0 on
    the diagonal."""
    xyz = np.asarray(points, dtype=np.float32)[:, :3].astype(np.float64)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    n = len(centers)
    near = np.full((n, n), -1, dtype=np.int64)
    members = [np.flatnonzero(point_node == i) for i in range(n)]
    for i in range(n):
        pi = xyz[members[i]]
        for j in range(n):
            if i == j or len(pi) == 0:
                continue
            mid = (centers[i] + centers[j]) * 0.5
            if not np.isfinite(mid).all():
                continue
            d = mid - pi
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            ok = np.isfinite(d2)
            if not ok.any():
                continue
            cand = np.flatnonzero(ok & (d2 <= d2[ok].min() * (1 + 1e-12)))
            if len(cand) > 1:
                fm = _frac3(mid)
                ex = [sum((a - b) ** 2 for a, b in zip(fm, _frac3(pi[c]))) for c in cand]
                cand = cand[[k for k, v in enumerate(ex) if v == min(ex)]]
            near[i, j] = members[i][cand[0]]
    dis = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            if near[i, j] < 0 or near[j, i] < 0:
                dis[i, j] = np.nan
            elif i < j:
                a, b = _frac3(xyz[near[i, j]]), _frac3(xyz[near[j, i]])
                dis[i, j] = sqrt_f64(sum((p - q) ** 2 for p, q in zip(a, b)))
            else:
                dis[i, j] = dis[j, i]
    return near, dis


def ulp_distance(a, b):
    """|a - b| in units of the spacing of float64 at b (elementwise; both finite)"""
    return np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.abs(np.asarray(b, dtype=np.float64)))


# ---- the kernel's float32 formulas, restated --------------------------------------------------------------------------

def f32_tol(tol):
    return np.float32(tol), np.float32(tol) * np.float32(tol)


def f32_d2(a, b):
    """(ex*ex + ey*ey) + ez*ez with every operation rounded to float32: the kernel's and the oracle's distance"""
    e = np.asarray(a, dtype=np.float32) - np.asarray(b, dtype=np.float32)
    ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
    return (ex * ex + ey * ey) + ez * ez


def f32_d2_reassociated(a, b):
    """ex*ex + (ey*ey + ez*ez), every operation rounded"""
    e = np.asarray(a, dtype=np.float32) - np.asarray(b, dtype=np.float32)
    ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
    return ex * ex + (ey * ey + ez * ez)


def round_f32(fr):
    """a Fraction rounded once to float32, ties to even"""
    c = np.float32(float(fr))
    best = None
    for v in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        err = abs(Fraction(float(v)) - fr)
        even = (int(np.float32(v).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, v)
    return np.float32(best[2])


def f32_d2_fused(a, b, form="chain"):
    """what a contracting compiler makes of the same expression, each fma rounded ONCE (exact product and sum as
    Fractions, then one rounding to float32).  "chain": fma(ez, ez, fma(ey, ey, ex*ex)); "inner_x" / "inner_y": only one
    product of the inner sum fused, fma(ex, ex, ey*ey) + ez*ez or fma(ey, ey, ex*ex) + ez*ez - the form hipcc gave
    the kernel before its distance was fenced with a contract(off) pragma."""
    e = (np.asarray(a, dtype=np.float32) - np.asarray(b, dtype=np.float32)).reshape(-1, 3)
    out = f32_d2(a, b).reshape(-1).copy()
    # the exact sum of squares, to ~1e-16: where the plain float32 form is within 1e-9 of it, a product was exact or
    # nearly so and the fused form - whose value lies between the two - rounds the same way; only the rest is redone
    exact = f64_d2(a, b).reshape(-1)
    for k in np.flatnonzero(np.abs(out.astype(np.float64) - exact) > 1e-9 * exact):
        ex, ey, ez = e[k]
        if form == "chain":
            t = round_f32(Fraction(float(ey)) ** 2 + Fraction(float(ex * ex)))
            out[k] = round_f32(Fraction(float(ez)) ** 2 + Fraction(float(t)))
        else:
            u, v = (ex, ey) if form == "inner_x" else (ey, ex)
            out[k] = round_f32(Fraction(float(u)) ** 2 + Fraction(float(v * v))) + ez * ez
    return out


def f64_d2(a, b):
    """the same expression on the same float32 coordinates, evaluated in float64"""
    e = np.asarray(a, dtype=np.float32).astype(np.float64) - np.asarray(b, dtype=np.float32).astype(np.float64)
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def cell_width(tol):
    return np.float32(tol) * np.float32(1.0001)


def cell_coord(v, tol):
    """floor(fl(v / fl(tol * 1.0001f))) in float32 -> int64"""
    return np.floor(np.asarray(v, dtype=np.float32) / cell_width(tol)).astype(np.int64)


def cell_key(c, cells):
    """the 62-bit key of the cell table: 5 bits of class, 19 bits per axis (offset binary, wrapped)"""
    k = [(int(v) + (1 << 18)) & 0x7FFFF for v in cells]
    return (int(c) << 57) | (k[0] << 38) | (k[1] << 19) | k[2]


def table_slots(p):
    h = 1024
    while h < 2 * p:
        h <<= 1
    return h


# ---- scan generators (all seeded) ---------------------------------------------------------------------------------------

def _scan(blocks, rng, shuffle=True):
    """[(xyz [k,3], raw id, instance id)] -> (points f32 [P,4], label u32 [P]) in shuffled point order"""
    xyz = np.concatenate([np.asarray(b[0], dtype=np.float64).reshape(-1, 3) for b in blocks]).astype(np.float32)
    lab = np.concatenate([np.full(len(np.asarray(b[0]).reshape(-1, 3)), b[1] | (b[2] << 16), dtype=np.uint32) for b in blocks])
    pts = np.concatenate((xyz, rng.random((len(lab), 1), dtype=np.float32)), axis=1)
    if shuffle:
        perm = rng.permutation(len(lab))
        pts, lab = pts[perm], lab[perm]
    return np.ascontiguousarray(pts), np.ascontiguousarray(lab)


def min_size_of(raw):
    return go.cluster_params(go.LEARNING_MAP[raw])[1]


def dumbbell_scan(a, b, raw, a_first, seed=0):
    """Dumbbells: for each k, ceil(min_size / 2) coincident points at float32 a[k] and as many at b[k].  The pair is a
    node (of min_size or min_size + 1 points) iff a[k] and b[k] are linked.  The caller keeps the dumbbells >= 3 tol apart.
    The kernel lets only the HIGHER-indexed point of a pair look the other one up, so the index order is fixed: where
    a_first[k], every point of a[k] has a lower index than every point of b[k], else the reverse (the low ends of all
    dumbbells come first, shuffled among themselves, then the high ends, shuffled).  Only the high end can find the
    link, and only in the cell offset `lookup_offsets` gives."""
    a, b = np.asarray(a, dtype=np.float32).reshape(-1, 3), np.asarray(b, dtype=np.float32).reshape(-1, 3)
    a_first = np.asarray(a_first, dtype=bool)[:, None]
    half = (min_size_of(raw) + 1) // 2
    rng = np.random.default_rng(seed)
    low, high = np.where(a_first, a, b), np.where(a_first, b, a)
    xyz = np.concatenate([np.repeat(end, half, axis=0)[rng.permutation(half * len(a))] for end in (low, high)])
    return _scan([(xyz, raw, 0)], rng, shuffle=False)


def lookup_offsets(a, b, a_first, tol):
    """the neighbour-cell offset in which the high end of each dumbbell finds the low end: cell(low) - cell(high)"""
    off = cell_coord(b, tol) - cell_coord(a, tol)
    return np.where(np.asarray(a_first, dtype=bool)[:, None], -off, off)


def emulation_pairs(points, tol):
    """every pair (o < p) in range by the float32 test, and the cell offset cell(o) - cell(p) in which p finds o"""
    from scipy.spatial import cKDTree
    xyz = np.asarray(points, dtype=np.float32)[:, :3]
    pairs = cKDTree(xyz.astype(np.float64)).query_pairs(float(tol) * 1.0001, output_type="ndarray")    # o = [:, 0] < p = [:, 1]
    pairs = pairs[f32_d2(xyz[pairs[:, 0]], xyz[pairs[:, 1]]) < f32_tol(tol)[1]]
    return pairs, cell_coord(xyz[pairs[:, 0]], tol) - cell_coord(xyz[pairs[:, 1]], tol)


def emulate_nodes(points, tol, min_size, dropped=(), pairs=None):
    """The kernel's pair enumeration for a scan of ONE Euclidean class, on the host: point p looks up the 27 cells around
    its own (minus the offsets in `dropped`) and links every point o < p there with float32 d2 < tol2; components of at
    least min_size points -> sorted list of (size, lowest point index).  With nothing dropped this is the reference's
    partition; it shows what a missed neighbour cell would do to a scan."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    pairs, off = emulation_pairs(points, tol) if pairs is None else pairs
    keep = np.abs(off).max(axis=1) <= 1
    for d in dropped:
        keep &= ~(off == np.asarray(d)).all(axis=1)
    pairs = pairs[keep]
    n = len(points)
    _, comp = connected_components(coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n)),
                                   directed=False)
    size = np.bincount(comp)
    first = np.full(len(size), n)
    np.minimum.at(first, comp, np.arange(n))
    return sorted((int(s), int(f)) for s, f in zip(size, first) if s >= min_size)


def threshold_candidates(tol, side=16, per_site=8, seed=0):
    """case a: side^3 * per_site candidate dumbbells (a, b) with |b - a| = tol * (1 +- 3e-7) in random directions; a on
    a lattice of 8 tol (side^3 sites around the origin, negative coordinates included) with a jitter of +-tol / 2, so
    that dumbbells of two DIFFERENT sites stay >= 5 tol apart -> (a, b, site number); a scan takes one per site."""
    rng = np.random.default_rng([seed, int(round(tol * 10))])
    count = side ** 3 * per_site
    site = np.stack(np.meshgrid(*[np.arange(side) - side // 2] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    site_no = np.tile(np.arange(side ** 3), per_site)
    site = site[site_no]
    a = (site * (8.0 * tol) + (rng.random((count, 3)) - 0.5) * tol).astype(np.float32)
    u = rng.normal(size=(count, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = tol * (1.0 + (rng.random((count, 1)) * 2 - 1) * 3e-7)
    b = (a.astype(np.float64) + u * r).astype(np.float32)
    return a, b, site_no


def classify(a, b, tol):
    """the groups of case a, from the kernel's formula -> dict of bool arrays (and `linked`)"""
    _, tol2 = f32_tol(tol)
    d2 = f32_d2(a, b)
    linked = d2 < tol2
    # a fused form differs from the plain one by the roundings of two operations at most: it can only flip a decision
    # within a few ulp of tol2, and only those candidates pay for its exact evaluation
    close = np.flatnonzero(np.abs(d2.astype(np.float64) - np.float64(tol2)) <= 4 * np.float64(np.spacing(tol2)))

    def flips(form):
        out = np.zeros(len(d2), dtype=bool)
        out[close] = (f32_d2_fused(a[close], b[close], form) < tol2) != linked[close]
        return out
    return {"linked": linked, "equal": d2 == tol2, "reassoc": (f32_d2_reassociated(a, b) < tol2) != linked,
            "fused": flips("chain"), "fused_inner": flips("inner_x") | flips("inner_y"),
            "f64": (f64_d2(a, b) < np.float64(np.float32(tol)) * np.float64(np.float32(tol))) != linked}


def cell_offsets(a, b, tol):
    return cell_coord(b, tol) - cell_coord(a, tol)


def axis_cases(tol):
    """case a by hand: spacing exactly tol (not linked) and nextafter(tol, 0) (linked) along +-x, +-y, +-z.  One end sits at
    0 on the spaced axis, so the spacing is exact in float32; the other two axes carry the dumbbell far from the rest."""
    t = np.float32(tol)
    a, b = [], []
    for k, (axis, sign, s) in enumerate((ax, sg, s) for ax in range(3) for sg in (1, -1) for s in (t, np.nextafter(t, np.float32(0)))):
        p = np.zeros(3, dtype=np.float32)
        p[(axis + 1) % 3] = np.float32(1000.0 + 16.0 * tol * k)
        p[(axis + 2) % 3] = np.float32(-1000.0)
        q = p.copy()
        q[axis] = np.float32(sign) * s
        a.append(p)
        b.append(q)
    return np.array(a), np.array(b)


def threshold_scan(tol, raw, per_group=30, others=60, seed=0):
    """cases a + b: the selected dumbbells of one tolerance -> (points, label, a, b, a_first).  Selected: up to
    `per_group` of each group of `classify`, up to 4 linked dumbbells per neighbour-cell offset, the linked dumbbells that
    straddle cells 0 / -1, `others` more at random, and the hand-made axis cases.  Index order (see dumbbell_scan): the
    dumbbells with one cell offset b - a alternate between a first and b first, so every offset is looked up from
    either end by some dumbbell."""
    a, b, site = threshold_candidates(tol, seed=seed)
    g = classify(a, b, tol)
    pick = np.zeros(len(a), dtype=bool)
    used = np.zeros(site.max() + 1, dtype=bool)

    def take(mask, limit):                                 # the first `limit` candidates of `mask` on sites still free
        got = 0
        for k in np.flatnonzero(mask):
            if got == limit:
                break
            if not used[site[k]]:
                used[site[k]] = pick[k] = True
                got += 1
    for name in ("equal", "reassoc", "fused", "fused_inner", "f64"):
        take(g[name], per_group)
    off = cell_offsets(a, b, tol)
    for o in np.unique(off[g["linked"]], axis=0):
        take(g["linked"] & (off == o).all(axis=1), 4)
    ca, cb = cell_coord(a, tol), cell_coord(b, tol)
    for ax in range(3):
        take(g["linked"] & (np.minimum(ca[:, ax], cb[:, ax]) == -1) & (np.maximum(ca[:, ax], cb[:, ax]) == 0), 4)
    take(np.random.default_rng(seed + 1).random(len(a)) < 0.05, others)
    ha, hb = axis_cases(tol)
    a, b = np.concatenate((a[pick], ha)), np.concatenate((b[pick], hb))
    _, group = np.unique(cell_offsets(a, b, tol), axis=0, return_inverse=True)
    group = group.reshape(-1) * 2 + (f32_d2(a, b) < f32_tol(tol)[1])
    a_first = np.zeros(len(a), dtype=bool)
    for v in np.unique(group):
        k = np.flatnonzero(group == v)
        a_first[k[::2]] = True
    pts, lab = dumbbell_scan(a, b, raw, a_first, seed=seed)
    return pts, lab, a, b, a_first


def far_scan(seed=0):
    """case b, far from the origin: dumbbells of the three tolerances around (+-40 km, +-40 km), where float32 is spaced
    2^-8 m, at |b - a| = tol * (1 +- 0.03), in dumbbell_scan's fixed index order -> (points, label, [(raw, tol, a, b, a_first)])"""
    rng = np.random.default_rng(seed)
    blocks, parts = [], []
    for raw, tol in ((TRUNK, 0.2), (FENCE, 0.5), (VEGETATION, 2.0)):
        a, b = [], []
        for sx in (-1, 1):
            for sy in (-1, 1):
                for k in range(6):
                    p = np.array([sx * 40000.0 + 16 * tol * k, sy * 40000.0, 3.0 * tol]) + (rng.random(3) - 0.5) * tol
                    u = rng.normal(size=3)
                    u /= np.linalg.norm(u)
                    a.append(p)
                    b.append(np.float32(p).astype(np.float64) + u * tol * (1 + (rng.random() * 2 - 1) * 0.03))
        a, b = np.array(a, dtype=np.float32), np.array(b, dtype=np.float32)
        a_first = np.arange(len(a)) % 2 == 0
        p, l = dumbbell_scan(a, b, raw, a_first, seed=seed)
        blocks.append((p, l))
        parts.append((raw, tol, a, b, a_first))
    return np.concatenate([p for p, _ in blocks]), np.concatenate([l for _, l in blocks]), parts


def alias_scan(seed=0):
    """case c: trunk clusters A (60 points) and B (70) whose x cells differ by exactly 2^19 - one 19-bit key - and C (55)
    that touches A -> (points, label, dict of the three float32 x positions and the y / z box)"""
    rng = np.random.default_rng(seed)
    tol = 0.2
    ax = np.float32(-52434.0)
    bx = np.float32(np.float64(ax) + 524288.0 * np.float64(cell_width(tol)))
    want = cell_coord(ax, tol) + (1 << 19)
    for _ in range(4096):                                  # walk float32 neighbours until the restated cell function agrees
        have = cell_coord(bx, tol)
        if have == want:
            break
        bx = np.nextafter(bx, np.float32(np.inf if have < want else -np.inf))
    cx = np.float32(np.float64(ax) + 0.12)

    def blob(x, count):                                    # y, z inside cell 0 (0 .. 0.20002 m): +-0.04 m around 0.1 m
        return np.stack((np.full(count, x, dtype=np.float64), 0.1 + (rng.random(count) - 0.5) * 0.08,
                         0.1 + (rng.random(count) - 0.5) * 0.08), axis=1)
    pts, lab = _scan([(blob(ax, 60), TRUNK, 0), (blob(bx, 70), TRUNK, 0), (blob(cx, 55), TRUNK, 0)], rng)
    return pts, lab, {"ax": ax, "bx": bx, "cx": cx}


def _blob(rng, centre, count, radius):
    return np.asarray(centre, dtype=np.float64) + (rng.random((count, 3)) - 0.5) * 2 * radius


def _lattice(count, width, origin):
    k = np.arange(count)
    return np.stack((origin[0] + (k % width) * 1.0, origin[1] + (k // width) * 1.0, np.full(count, origin[2])), axis=1)


def size_scan_euclidean(seed=0):
    """case d, first scan: for every Euclidean node class blobs of min_size - 1, min_size and min_size + 1 points
    (radius 0.1 tol, 40 m apart), and for class 17 (raw 72, 2 m) planar 1 m lattices of 50 000 and 50 001 points."""
    rng = np.random.default_rng(seed)
    blocks = []
    for row, (c, raw) in enumerate(sorted(EUCLID_RAW.items())):
        tol, mn = go.cluster_params(c)
        for col, count in enumerate((mn - 1, mn, mn + 1)):
            blocks.append((_blob(rng, (-200.0 - 40 * col, 40.0 * row, 1.0), count, 0.1 * tol), raw, 0))
    blocks.append((_lattice(50000, 250, (0.0, 0.0, 0.0)), 72, 0))
    blocks.append((_lattice(50001, 250, (400.0, 0.0, 0.0)), 72, 0))
    return _scan(blocks, rng)


def size_scan_instances(seed=0):
    """case d, second scan (a class is either instance-labelled or Euclidean in one scan): class 1 (raw 10) with
    instance groups of 20, 21 and 50 001 points (a lattice; instance groups have no maximum), next to Euclidean blobs
    of two other classes."""
    rng = np.random.default_rng(seed)
    blocks = [(_blob(rng, (-50.0, 0.0, 0.0), 20, 1.0), 10, 4), (_blob(rng, (-50.0, 20.0, 0.0), 21, 1.0), 10, 2),
              (_lattice(50001, 250, (0.0, 0.0, 0.0)), 10, 3),
              (_blob(rng, (-50.0, 60.0, 0.0), 49, 0.02), TRUNK, 0), (_blob(rng, (-50.0, 80.0, 0.0), 50, 0.02), TRUNK, 0),
              (_blob(rng, (-50.0, 100.0, 0.0), 100, 0.05), FENCE, 0)]
    return _scan(blocks, rng)


N_RAW = len(go.remap_lut())          # 359: the reference's lookup table length


def every_label_scan(inst, seed=0):
    """case e: one blob of 320 points (radius 0.02 m) per raw id 0 .. 358, 20 m apart, all with instance id `inst`"""
    rng = np.random.default_rng(seed)
    blocks = [(_blob(rng, (20.0 * (raw % 20) - 200.0, 20.0 * (raw // 20) - 180.0, 0.5), 320, 0.02), raw, inst)
              for raw in range(N_RAW)]
    return _scan(blocks, rng)


def mixed_mode_scan(seed=0):
    """case e, third run: the modes of one class next to each other (see test_cluster_host for what each part proves)"""
    rng = np.random.default_rng(seed)
    blocks = [
        # class 5 (raw 13) with instance ids {0, 5, 65535}; its id-0 points are two blobs 50 m apart -> ONE node of 60
        (_blob(rng, (0.0, 0.0, 0.0), 30, 0.3), 13, 0), (_blob(rng, (50.0, 0.0, 0.0), 30, 0.3), 13, 0),
        (_blob(rng, (0.0, 20.0, 0.0), 40, 0.3), 13, 5), (_blob(rng, (0.0, 40.0, 0.0), 25, 0.3), 13, 65535),
        # the same instance id under two classes -> two nodes
        (_blob(rng, (100.0, 0.0, 0.0), 30, 0.3), 10, 7), (_blob(rng, (100.0, 20.0, 0.0), 35, 0.3), 18, 7),
        # raw 10 and raw 252 with one instance id: both are class 1 -> one node of 30 (15 alone would be dropped)
        (_blob(rng, (100.0, 40.0, 0.0), 15, 0.3), 10, 9), (_blob(rng, (100.0, 43.0, 0.0), 15, 0.3), 252, 9),
        # classes whose only instance id is 0: the Euclidean path - two pole blobs 50 m apart stay two nodes
        (_blob(rng, (200.0, 0.0, 0.0), 60, 0.02), TRUNK, 0),
        (_blob(rng, (200.0, 20.0, 0.0), 100, 0.02), 80, 0), (_blob(rng, (250.0, 20.0, 0.0), 101, 0.02), 80, 0),
    ]
    return _scan(blocks, rng)


def order_scan(seed=0):
    """case f: fence clusters of sizes 160, 140, five of 120 and one of 105, the five equal ones with their lowest
    point indices in the order EQUAL_ORDER; car instance groups whose sizes descend while their ids ascend.
    -> (points, label, the blob number of every point)"""
    rng = np.random.default_rng(seed)
    sizes = [160, 120, 120, 140, 120, 120, 105, 120]
    blobs = [_blob(rng, (30.0 * k, 0.0, 0.0), s, 0.1) for k, s in enumerate(sizes)]
    inst = [(2, 90), (5, 70), (9, 50), (11, 30)]
    xyz = np.concatenate(blobs + [_blob(rng, (30.0 * k, 50.0, 0.0), s, 1.0) for k, (_, s) in enumerate(inst)])
    blob = np.concatenate([np.full(s, k) for k, s in enumerate(sizes)] + [np.full(s, 100 + i) for i, s in inst])
    lab = np.concatenate([np.full(sum(sizes), FENCE, dtype=np.uint32)] + [np.full(s, 10 | (i << 16), dtype=np.uint32) for i, s in inst])
    # the first five points: one of each equal-sized blob, in EQUAL_ORDER; everything else shuffled behind them
    first = [int(np.flatnonzero(blob == k)[0]) for k in EQUAL_ORDER]
    rest = np.setdiff1d(np.arange(len(blob)), first)
    order = np.concatenate((first, rng.permutation(rest)))
    pts = np.concatenate((xyz.astype(np.float32), rng.random((len(blob), 1), dtype=np.float32)), axis=1)
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(lab[order]), blob[order]


EQUAL_ORDER = [5, 1, 7, 2, 4]        # blob numbers of order_scan's five 120-point clusters, by lowest point index


def chain_scan(count=20000, row=200, gap_row=None):
    """case g: a trunk-class serpentine chain of `count` points, every step 0.19 m (< 0.2 m): rows of `row` points along
    x, alternately forwards and backwards, 0.38 m apart in y, joined at their ends by one point half way.  (Rows 0.19 m
    apart would link everywhere and make a sheet that no single gap can cut; at 0.38 m the rows do not link, yet about
    half of them lie in neighbouring 0.20002 m cells, so the neighbour lookups of one row meet the points of the next
    and only the distance test keeps them apart.)  With `gap_row` (an even row) the
    step between that row's first point (x = 0) and its second is exactly 0.2f - not a link - and every later point is
    shifted by the same amount in x: two chains.  -> xyz float32 [count, 3] in chain order, and the length of the first part"""
    pos, split = [], None
    r = 0
    while len(pos) < count:
        xs = np.arange(row) * 0.19
        xs = xs if r % 2 == 0 else xs[::-1]
        for k, x in enumerate(xs):
            if gap_row is not None and r == gap_row and k == 1:
                split = len(pos)
            pos.append((x, 0.38 * r, 0.0))
        pos.append((xs[-1], 0.38 * r + 0.19, 0.0))
        r += 1
    xyz = np.array(pos[:count], dtype=np.float64).astype(np.float32)
    if split is not None:
        assert xyz[split - 1, 0] == 0
        shift = np.float64(np.float32(0.2)) - np.float64(xyz[split, 0])
        xyz[split:, 0] = (xyz[split:, 0].astype(np.float64) + shift).astype(np.float32)
        xyz[split, 0] = np.float32(0.2)
    return xyz, split


def chain_points(xyz, order):
    pts = np.concatenate((xyz, np.zeros((len(xyz), 1), dtype=np.float32)), axis=1)[order]
    return np.ascontiguousarray(pts), np.full(len(xyz), TRUNK, dtype=np.uint32)


def occupancy_scan(isolated, seed=0):
    """case h: `isolated` trunk points, one per cell (a 1 m lattice with +-0.2 m of jitter: >= 0.6 m apart), and two
    dumbbells among them (one linked at 0.19 m, one not at 0.21 m) -> (points, label); isolated + 100 points"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(isolated)))
    k = np.arange(isolated)
    iso = np.stack((k % side + 0.5, k // side + 0.5, np.zeros(isolated)), axis=1) + (rng.random((isolated, 3)) - 0.5) * 0.4
    a = np.array([[2.0, 3.0, 5.0], [side - 2.0, side - 3.0, -5.0]])
    b = a + np.array([[0.19, 0.0, 0.0], [0.0, 0.21, 0.0]])
    return _scan([(iso, TRUNK, 0), (np.repeat(a, 25, axis=0), TRUNK, 0), (np.repeat(b, 25, axis=0), TRUNK, 0)], rng)


def instance_scan(ids, per=21, seed=0):
    """case i: class 1 (raw 10) with instance ids 1 .. `ids` of `per` points each, scattered"""
    rng = np.random.default_rng(seed)
    inst = np.repeat(np.arange(1, ids + 1, dtype=np.uint32), per)
    xyz = (rng.random((len(inst), 3)) - 0.5) * 100
    perm = rng.permutation(len(inst))
    pts = np.concatenate((xyz, rng.random((len(inst), 1))), axis=1).astype(np.float32)[perm]
    return np.ascontiguousarray(pts), np.ascontiguousarray((np.uint32(10) | (inst << 16))[perm])


def poisoned_scans(seed=3, scale=0.5):
    """case j: synth.labelled_scan with non-finite values planted -> (points, label, {name: (points', planted)})
    where `planted` lists (point index, column, value).  "car_nan_x": one NaN x in car instance 3; "truck_inf_z": +inf z in
    the truck; "euclid_road": NaN / +-inf in buildings, vegetation, trunks, terrain and the road; "remission": NaN in
    column 3 only."""
    from sg_pr_amd import synth
    pts, lab = synth.labelled_scan(seed=seed, scale=scale)
    rng = np.random.default_rng(seed)

    def some(raw, inst, k):
        return rng.choice(np.flatnonzero(lab == np.uint32(raw | (inst << 16))), k, replace=False).tolist()
    plans = {
        "car_nan_x": [(some(10, 3, 1)[0], 0, np.nan)],
        "truck_inf_z": [(some(18, 1, 1)[0], 2, np.inf)],
        "euclid_road": [(p, col, v) for raws, col, v in (((50, 70), 0, np.nan), ((71, 72), 1, np.inf), ((40, 50), 2, -np.inf))
                        for raw in raws for p in some(raw, 0, 2)],
        "remission": [(p, 3, np.nan) for p in rng.choice(len(lab), 50, replace=False).tolist()],
    }
    out = {}
    for name, plan in plans.items():
        bad = pts.copy()
        for p, col, v in plan:
            bad[p, col] = v
        out[name] = (bad, plan)
    return pts, lab, out


def dyadic_edge_case(swap=False):
    """case k: four hand-made nodes on multiples of 1/8 m (every product and sum exact in float64) -> (points f32 [P,3],
    point_node, centers).  The centres are free inputs of sgpr_graph_edges; they are chosen so that
      * node 0 has two points, (1, 1, 0) and (1, -1, 0), equidistant from the midpoint (0, 0, 0) of nodes 0 and 1, whose
        distances to node 1's only point (-1, 1, 0) differ (2 and sqrt 8): the lower scan index must win (`swap`
        exchanges the two);
      * nodes 2 and 3 are single points (32, 0, 0) and (35, 4, 0): exactly 5.0 apart."""
    p0 = [(1.0, 1.0, 0.0), (1.0, -1.0, 0.0)]
    if swap:
        p0 = p0[::-1]
    pts = np.array(p0 + [(-1.0, 1.0, 0.0), (32.0, 0.0, 0.0), (35.0, 4.0, 0.0), (1.125, 0.0, 0.25)], dtype=np.float32)
    point_node = np.array([0, 0, 1, 2, 3, -1], dtype=np.int32)
    centers = np.array([(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (32.0, 0.0, 0.0), (35.0, 4.0, 0.0)], dtype=np.float64)
    return pts, point_node, centers
