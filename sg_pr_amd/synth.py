"""Seeded synthetic semantic graphs for the bench / parity configurations.

The reference ships only three real graphs (data/{0,3,250}.json); KITTI graph
JSONs live off-repo (reference README.md:54).  These generators follow the
specification in SURVEY.md §8(d) (configs 2, 3 and 5 of BASELINE.json): the
packed wire format is what `SGTrainer.transfer_to_torch` (reference
sg_net.py:241-310) produces before the one-hot expansion, i.e.

    centers  float32 [G, N, 3]   zero for padded slots        (sg_net.py:262)
    labels   int32   [G, N]      -1   for padded slots        (sg_net.py:260)

Every graph keeps >= k padded slots so that kNN ties are only ever between
feature-identical nodes (SURVEY.md §7 finding 3) - the regime in which the
reference itself is deterministic across torch.topk implementations.

numpy only; no torch import here.
"""
import numpy as np

NUM_LABELS = 12

# label histogram of the three shipped graphs (classes 0,3,5..11 dominant)
_KITTI_LABEL_P = np.array([28, 0, 0, 10, 0, 16, 7, 25, 12, 4, 7, 3], dtype=np.float64)
_KITTI_LABEL_P /= _KITTI_LABEL_P.sum()


def make_graphs(num_graphs, node_num, n_real_lo, n_real_hi, seed, kitti_like=False):
    """Return (centers f32 [G,N,3], labels i32 [G,N], n_real i32 [G])."""
    rng = np.random.default_rng(seed)
    centers = np.zeros((num_graphs, node_num, 3), dtype=np.float32)
    labels = -np.ones((num_graphs, node_num), dtype=np.int32)
    n_real = rng.integers(n_real_lo, n_real_hi + 1, size=num_graphs).astype(np.int32)
    for g in range(num_graphs):
        n = int(n_real[g])
        xy = rng.uniform(-50.0, 50.0, size=(n, 2))
        z = rng.uniform(-2.0, 1.0, size=(n, 1))
        if kitti_like:
            lab = rng.choice(NUM_LABELS, size=n, p=_KITTI_LABEL_P)
        else:
            lab = rng.integers(0, NUM_LABELS, size=n)
        lab.sort()
        centers[g, :n, :2] = xy
        centers[g, :n, 2:] = z
        labels[g, :n] = lab
    return centers, labels, n_real


def config2_pairs(seed=0, batch=128, node_num=64):
    """BASELINE config 2: `batch` pairs, N=64 slots, k=10, n_real ~ U{20..54}.

    Graph 2b is side 1 and graph 2b+1 is side 2 of pair b."""
    return make_graphs(2 * batch, node_num, 20, node_num - 10, seed)


def config5_pairs(seed=0, batch=1024, node_num=256):
    """BASELINE config 5 (stress): N=256, k=20, n_real ~ U{100..236}."""
    return make_graphs(2 * batch, node_num, 100, node_num - 20, seed)


def kitti_like_sequence(num_graphs=4541, node_num=100, seed=0):
    """BASELINE config 3 stand-in: KITTI-00-sized sequence (4541 frames).

    n_real ~ U{25..60}, shipped-graph label histogram, poses = planar random
    walk with revisits so that d<=3 m and d>=20 m pairs both exist.
    Returns (centers, labels, n_real, poses f64 [G,12])."""
    centers, labels, n_real = make_graphs(num_graphs, node_num, 25, 60, seed, kitti_like=True)
    rng = np.random.default_rng(seed + 7919)
    heading = np.cumsum(rng.normal(0.0, 0.05, size=num_graphs))
    step = np.stack([np.cos(heading), np.sin(heading)], axis=1)  # 1 m per frame
    xz = np.cumsum(step, axis=0)
    # revisit: the last third of the sequence re-drives the first third (+noise)
    third = num_graphs // 3
    if third > 0:
        xz[-third:] = xz[:third] + rng.normal(0.0, 0.5, size=(third, 2))
    poses = np.zeros((num_graphs, 12), dtype=np.float64)
    poses[:, 0] = poses[:, 5] = poses[:, 10] = 1.0
    poses[:, 3] = xz[:, 0]   # x   (utils.py:36 uses pose[3], pose[11])
    poses[:, 11] = xz[:, 1]  # z
    return centers, labels, n_real, poses


def world_sequence(num_graphs=4541, node_num=100, seed=0, sensor_range=50.0, center_noise=0.15, dropout=0.12,
                   density=0.0062, region=60.0, mix_alpha=3.0):
    """A KITTI-00-sized sequence whose graphs come from ONE world, so that revisits look alike and the
    precision-recall curve of the score matrix means something (`kitti_like_sequence` draws every graph
    independently of its pose: its F1-max is chance).

    The world is a fixed set of landmarks (label from the shipped-graph histogram, position uniform over the
    trajectory's bounding box + sensor_range, height in [-2, 1] like the shipped graphs).  The vehicle drives a
    planar random walk at 1 m per frame; the last third re-drives the first third (lateral offset ~0.5 m, heading
    within a few degrees).  Frame t sees the landmarks within `sensor_range` of its pose, in the sensor frame
    (x forward, y left, z up: the frame the shipped graphs' centres are in), each one dropped with probability
    `dropout` and its centre jittered by N(0, center_noise) m - what a per-frame clustering does to a real
    object.  At most node_num - 40 nodes are kept (nearest first), i.e. >= 40 padded slots: the tie regime stays
    the reference's deterministic one.  Nodes are listed label-ascending like the shipped graphs.
    Returns (centers f32 [G,N,3], labels i32 [G,N], n_real i32 [G], poses f64 [G,12]) - the KITTI 3x4 pose with
    the heading as a rotation about the camera's y axis; utils.py:36 reads entries 3 (x) and 11 (z)."""
    rng = np.random.default_rng(seed + 104729)
    G = int(num_graphs)
    heading = np.cumsum(rng.normal(0.0, 0.05, size=G))
    xz = np.cumsum(np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0)
    third = G // 3
    if third > 0:
        xz[-third:] = xz[:third] + rng.normal(0.0, 0.5, size=(third, 2))
        heading[-third:] = heading[:third] + rng.normal(0.0, 0.03, size=third)
    lo, hi = xz.min(0) - sensor_range, xz.max(0) + sensor_range
    n_land = max(int(density * float(np.prod(hi - lo))), 1)
    land_xz = rng.uniform(lo, hi, size=(n_land, 2))
    land_h = rng.uniform(-2.0, 1.0, size=n_land)
    # places differ: every `region` x `region` m cell of the world has its own label mix (a Dirichlet draw around the
    # shipped-graph histogram) - a street of buildings and fences here, vegetation and trunks there
    reg = np.floor((land_xz - lo) / region).astype(np.int64)
    nreg = reg.max(0) + 1
    mix = rng.dirichlet(_KITTI_LABEL_P * mix_alpha + 1e-3, size=int(nreg[0] * nreg[1]))
    cum = np.cumsum(mix[reg[:, 0] * nreg[1] + reg[:, 1]], axis=1)
    land_lab = np.minimum((rng.random(n_land)[:, None] > cum).sum(1), NUM_LABELS - 1)
    # landmarks nowhere near the trajectory are never seen: drop them before the per-frame search
    cell = np.floor(xz / sensor_range).astype(np.int64)
    near = set()
    for dx in (-1, 0, 1):
        for dz in (-1, 0, 1):
            near.update(map(tuple, cell + (dx, dz)))
    keep = np.fromiter((tuple(c) in near for c in np.floor(land_xz / sensor_range).astype(np.int64)), bool, n_land)
    land_xz, land_h, land_lab = land_xz[keep], land_h[keep], land_lab[keep]
    max_real = max(node_num - 40, 1)
    centers = np.zeros((G, node_num, 3), dtype=np.float32)
    labels = -np.ones((G, node_num), dtype=np.int32)
    n_real = np.zeros(G, dtype=np.int32)
    for t in range(G):
        d = land_xz - xz[t]
        r2 = (d * d).sum(1)
        seen = np.flatnonzero(r2 <= sensor_range * sensor_range)
        seen = seen[rng.random(seen.size) >= dropout]
        if seen.size > max_real:
            seen = seen[np.argsort(r2[seen], kind="stable")[:max_real]]
        c, s = np.cos(heading[t]), np.sin(heading[t])
        fwd = d[seen, 0] * c + d[seen, 1] * s
        left = -d[seen, 0] * s + d[seen, 1] * c
        pts = np.stack([fwd, left, land_h[seen]], axis=1) + rng.normal(0.0, center_noise, size=(seen.size, 3))
        order = np.argsort(land_lab[seen], kind="stable")
        n = seen.size
        centers[t, :n] = pts[order]
        labels[t, :n] = land_lab[seen][order]
        n_real[t] = n
    poses = np.zeros((G, 12), dtype=np.float64)
    poses[:, 0] = poses[:, 10] = np.cos(heading)
    poses[:, 2] = np.sin(heading)
    poses[:, 8] = -np.sin(heading)
    poses[:, 5] = 1.0
    poses[:, 3] = xz[:, 0]
    poses[:, 11] = xz[:, 1]
    return centers, labels, n_real, poses


def _se2_compose(a, b):
    """a o b (b first) on planar poses [..., 4] = (c, s, x, y)"""
    return np.stack((a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1], a[..., 1] * b[..., 0] + a[..., 0] * b[..., 1],
                     a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2],
                     a[..., 1] * b[..., 2] + a[..., 0] * b[..., 3] + a[..., 3]), axis=-1)


def _se2_inverse(a):
    return np.stack((a[..., 0], -a[..., 1], -(a[..., 0] * a[..., 2] + a[..., 1] * a[..., 3]),
                     a[..., 1] * a[..., 2] - a[..., 0] * a[..., 3]), axis=-1)


def _se2(yaw, x, y):
    yaw, x, y = np.broadcast_arrays(np.asarray(yaw, dtype=np.float64), x, y)
    return np.stack((np.cos(yaw), np.sin(yaw), x, y), axis=-1).astype(np.float64)


def _random_walk(rng, S):
    """the planar trajectory of closure_world and drift_world: 1 m per scan, the heading a random walk of 0.05 rad"""
    heading = np.cumsum(rng.normal(0.0, 0.05, size=S))
    xy = np.cumsum(np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0)
    return heading, xy


def closure_world(seed, scans=600, closures=400, outlier_frac=0.5, alias=30, noise_t=0.15, noise_yaw=0.01):
    """A planted set of loop closures between two drives, for the pairwise-consistency stage.

    Two drives of one planar random-walk trajectory (1 m per scan): the second is offset by N(0, 0.5) m per scan and its
    odometry is expressed in a frame of its own, rotated by 1.1 rad and shifted by (40, -25) - the two sessions' frames
    are unrelated, as in a multi-session map.  A closure pairs a row scan of drive 1 with a column scan of drive 2 and
    carries T, a point of the row scan into the column scan.  True closures pair scans within +-2 indices and carry the
    true transform perturbed by N(0, noise_yaw) rad and N(0, noise_t) m; outliers pair random scans with random
    transforms; `alias` of the outliers are rebuilt to agree on ONE wrong alignment of the two frames (a perceptually
    aliased place: consistent with each other, inconsistent with the truth), with the same noise.
    -> dict: rows, cols int32 [C]; T float64 [C,4] (c, s, tx, ty); Xr, Xc float64 [scans,4] planar odometry (c, s, x,
    y); planted bool [C] (a true closure); aliased bool [C].  Closures are shuffled.  numpy only."""
    rng = np.random.default_rng(seed + 15485863)
    S, C = int(scans), int(closures)
    heading, xy = _random_walk(rng, S)
    X1 = _se2(heading, xy[:, 0], xy[:, 1])
    xy2 = xy + rng.normal(0.0, 0.5, size=(S, 2))
    X2 = _se2(heading + rng.normal(0.0, 0.03, size=S), xy2[:, 0], xy2[:, 1])        # drive 2 in drive 1's frame
    frame = _se2(1.1, 40.0, -25.0)
    Xc = _se2_compose(frame, X2)
    n_out = min(C, int(round(float(outlier_frac) * C)))
    n_alias = min(int(alias), n_out)
    planted = np.zeros(C, dtype=bool)
    planted[n_out:] = True
    aliased = np.zeros(C, dtype=bool)
    aliased[:n_alias] = True
    rows = rng.integers(0, S, size=C)
    cols = np.where(planted, np.clip(rows + rng.integers(-2, 3, size=C), 0, S - 1), rng.integers(0, S, size=C))

    def noisy(t):
        return _se2_compose(_se2(rng.normal(0.0, noise_yaw, size=C), rng.normal(0.0, noise_t, size=C),
                                 rng.normal(0.0, noise_t, size=C)), t)

    truth = noisy(_se2_compose(_se2_inverse(X2[cols]), X1[rows]))
    wrong = _se2_compose(_se2(0.4, 15.0, -8.0), X1[rows])                            # ... if the frames were aligned so
    fake = noisy(_se2_compose(_se2_inverse(X2[cols]), wrong))
    rand = _se2(rng.uniform(-np.pi, np.pi, size=C), rng.uniform(-30.0, 30.0, size=C), rng.uniform(-30.0, 30.0, size=C))
    T = np.where(planted[:, None], truth, np.where(aliased[:, None], fake, rand))
    perm = rng.permutation(C)
    return {"rows": rows[perm].astype(np.int32), "cols": cols[perm].astype(np.int32),
            "T": np.ascontiguousarray(T[perm]), "Xr": X1, "Xc": Xc, "planted": planted[perm], "aliased": aliased[perm]}


def drift_world(seed, scans=300, sessions=2, closures=120, noise_t=0.15, noise_yaw=0.01, odo_yaw=0.004, odo_t=0.03):
    """A multi-session map with drifting odometry and true loop closures, for the pose-graph stage.

    `sessions` drives of closure_world's trajectory (1 m per scan), each jittered by N(0, 0.5) m and N(0, 0.03) rad.
    The odometry of a drive is integrated from its true relative motions, each perturbed by N(0, odo_yaw) rad and
    N(0, odo_t) m, starting in a frame of its own (drive d: rotated by 1.1 d rad, shifted by (40 d, -25 d)) - so every
    drive drifts and the frames are unrelated.  A closure joins a scan of one drive to a scan within +-2 indices of a
    different drive and carries T, a point of scan rows[p] into scan cols[p], with closure_world's noise.
    -> dict: truth, odom float64 [sessions * scans, 4] planar poses (c, s, x, y) of the stacked map; starts int32
    [sessions]; rows, cols int32 [C] (indices into the stacked map); T float64 [C,4].  numpy only."""
    rng = np.random.default_rng(seed + 32452843)
    S, D, C = int(scans), int(sessions), int(closures)
    heading, xy = _random_walk(rng, S)
    truth, odom = [], []
    for d in range(D):
        xyd = xy + rng.normal(0.0, 0.5, size=(S, 2))
        Xt = _se2(heading + rng.normal(0.0, 0.03, size=S), xyd[:, 0], xyd[:, 1])
        rel = _se2_compose(_se2_inverse(Xt[:-1]), Xt[1:])
        rel = _se2_compose(rel, _se2(rng.normal(0.0, odo_yaw, size=S - 1), rng.normal(0.0, odo_t, size=S - 1),
                                     rng.normal(0.0, odo_t, size=S - 1)))
        Xo = np.empty((S, 4), dtype=np.float64)
        Xo[0] = _se2_compose(_se2(1.1 * d, 40.0 * d, -25.0 * d), Xt[0])
        for k in range(S - 1):
            Xo[k + 1] = _se2_compose(Xo[k], rel[k])
        truth.append(Xt)
        odom.append(Xo)
    truth, odom = np.concatenate(truth), np.concatenate(odom)
    a = rng.integers(0, D, size=C)
    b = (a + rng.integers(1, max(D, 2), size=C)) % D if D > 1 else a
    i = rng.integers(0, S, size=C)
    j = np.clip(i + rng.integers(-2, 3, size=C), 0, S - 1)
    rows, cols = a * S + i, b * S + j
    T = _se2_compose(_se2(rng.normal(0.0, noise_yaw, size=C), rng.normal(0.0, noise_t, size=C),
                          rng.normal(0.0, noise_t, size=C)), _se2_compose(_se2_inverse(truth[cols]), truth[rows]))
    return {"truth": truth, "odom": odom, "starts": (np.arange(D) * S).astype(np.int32), "rows": rows.astype(np.int32),
            "cols": cols.astype(np.int32), "T": np.ascontiguousarray(T)}


def localize_world(seed, map_scans=600, queries=200, k=8, true_frac=0.4, alias_frac=0.25, alias=4, noise_t=0.15,
                   noise_yaw=0.01, odo_yaw=0.004, odo_t=0.03):
    """A map, a query drive and candidate lists with planted truths and aliases, for the localisation stage (DESIGN.md
    §26).

    The map is closure_world's trajectory (1 m per scan) with its true poses.  The queries re-drive a random stretch of
    it, jittered by N(0, 0.5) m and N(0, 0.03) rad; their odometry is integrated from the true relative motions, each
    perturbed by N(0, odo_yaw) rad and N(0, odo_t) m, in a frame of its own (rotated by 1.1 rad, shifted by (40, -25)),
    as in drift_world.  Every query has k candidates (col, T: a point of the query scan into map scan col).  A candidate
    is true with probability true_frac: its column lies within +-2 of the query's map index and T is the true transform
    perturbed by N(0, noise_yaw) rad and N(0, noise_t) m, as in closure_world.  The rest are random columns with random
    transforms (+-30 m, any yaw).  In a share alias_frac of the queries the first `alias` false candidates are rebuilt
    to agree on ONE wrong pose, drawn per query anywhere in the map's bounding box, with the same noise: they agree with
    one another within a scan, and, not moving with the odometry, with nothing across scans.
    -> dict: map float64 [map_scans,4]; truth, odom float64 [queries,4] (c, s, x, y); index int32 [queries] (the map
    scan each query re-drives); cols int32 [queries,k]; T float64 [queries,k,4]; planted, aliased bool [queries,k].
    numpy only."""
    rng = np.random.default_rng(seed + 49979687)
    M, Q, K = int(map_scans), int(queries), int(k)
    heading, xy = _random_walk(rng, M)
    world = _se2(heading, xy[:, 0], xy[:, 1])
    index = int(rng.integers(0, M - Q + 1)) + np.arange(Q)
    xyq = xy[index] + rng.normal(0.0, 0.5, size=(Q, 2))
    truth = _se2(heading[index] + rng.normal(0.0, 0.03, size=Q), xyq[:, 0], xyq[:, 1])
    rel = _se2_compose(_se2_inverse(truth[:-1]), truth[1:])
    rel = _se2_compose(rel, _se2(rng.normal(0.0, odo_yaw, size=Q - 1), rng.normal(0.0, odo_t, size=Q - 1),
                                 rng.normal(0.0, odo_t, size=Q - 1)))
    odom = np.empty((Q, 4), dtype=np.float64)
    odom[0] = _se2_compose(_se2(1.1, 40.0, -25.0), truth[0])
    for i in range(Q - 1):
        odom[i + 1] = _se2_compose(odom[i], rel[i])
    planted = rng.random((Q, K)) < float(true_frac)
    near = np.clip(index[:, None] + rng.integers(-2, 3, size=(Q, K)), 0, M - 1)
    cols = np.where(planted, near, rng.integers(0, M, size=(Q, K)))
    false_rank = np.cumsum(~planted, axis=1) - 1                               # 0, 1, ... over a query's false candidates
    aliased = (~planted) & (false_rank < int(alias)) & (rng.random(Q) < float(alias_frac))[:, None]
    lo, hi = xy.min(0), xy.max(0)
    wrong = _se2(rng.uniform(-np.pi, np.pi, size=Q), rng.uniform(lo[0], hi[0], size=Q), rng.uniform(lo[1], hi[1], size=Q))

    def noisy(t):
        return _se2_compose(_se2(rng.normal(0.0, noise_yaw, size=(Q, K)), rng.normal(0.0, noise_t, size=(Q, K)),
                                 rng.normal(0.0, noise_t, size=(Q, K))), t)

    to_col = _se2_inverse(world[cols])
    true_T = noisy(_se2_compose(to_col, truth[:, None, :]))
    fake_T = noisy(_se2_compose(to_col, wrong[:, None, :]))
    rand_T = _se2(rng.uniform(-np.pi, np.pi, size=(Q, K)), rng.uniform(-30.0, 30.0, size=(Q, K)),
                  rng.uniform(-30.0, 30.0, size=(Q, K)))
    T = np.where(planted[..., None], true_T, np.where(aliased[..., None], fake_T, rand_T))
    return {"map": world, "truth": truth, "odom": odom, "index": index.astype(np.int32), "cols": cols.astype(np.int32),
            "T": np.ascontiguousarray(T), "planted": planted, "aliased": aliased}


def dense_features(centers, labels, num_labels=NUM_LABELS):
    """Packed (centers, labels) -> the reference's dense `B x (3+L) x N` float32
    tensor (sg_net.py:274-298): xyz rows then a one-hot block, all-zero for -1."""
    g, n, _ = centers.shape
    out = np.zeros((g, 3 + num_labels, n), dtype=np.float32)
    out[:, :3, :] = centers.transpose(0, 2, 1)
    gi, ni = np.nonzero(labels >= 0)
    out[gi, 3 + labels[gi, ni], ni] = 1.0
    return out


def effective_nodes(centers, labels, k):
    """Slots the engine actually processes per graph: of the m trailing slots identical to the last one
    (zero padding) a single representative is kept when m >= k, all m otherwise ("duplicate
    slots").  Returns int32 [G]."""
    g, n = labels.shape
    same = (labels == labels[:, -1:]) & (centers == centers[:, -1:, :]).all(-1)     # [G, N]
    differs = ~same
    last = np.where(differs.any(1), n - 1 - np.argmax(differs[:, ::-1], axis=1), -1)
    nd = last + 1
    m = n - nd
    return (nd + np.where((m >= k) & (m > 1), 1, m)).astype(np.int32)


def labelled_scan(seed=0, scale=1.0):
    """A SemanticKITTI-like labelled LiDAR scan for the upstream graph generator (the reference ships
    no scans): points float32 [P,4] (x, y, z, remission) and labels uint32 [P] (raw semantic id | instance id << 16,
    the .label format gen_label_graph.py:204-227 reads).  Contains every per-class mode of gen_labels: road / parking
    (one cluster, never a node), discarded classes, instance-labelled vehicles (incl. an instance of <= 20 points and
    points with instance id 0), and Euclidean classes at all three tolerances with objects above and below their
    minimum sizes.  `scale` multiplies the point counts (1.0 -> ~70 k points).  Point order is shuffled."""
    rng = np.random.default_rng(seed)
    pts, lab = [], []

    def add(xyz, sem, inst=0):
        pts.append(np.asarray(xyz, dtype=np.float64))
        lab.append(np.full(len(xyz), sem | (inst << 16), dtype=np.uint32))

    def n(x):
        return max(1, int(round(x * scale)))

    def box(c, size, count):
        return np.asarray(c) + (rng.random((count, 3)) - 0.5) * np.asarray(size)

    add(box((0, 0, -1.7), (100, 8, 0.05), n(15000)), 40)                       # road
    add(box((20, 9, -1.7), (12, 6, 0.05), n(1500)), 44)                        # parking
    add(box((0, 6.5, -1.6), (100, 3, 0.05), n(5000)), 48)                      # sidewalk: two strips > 2 m apart
    add(box((0, -6.5, -1.6), (100, 3, 0.05), n(5000)), 48)
    add(box((60, 20, -1.6), (2, 2, 0.05), n(120)), 48)                         # ... and a patch below min size 300
    for b in range(6):                                                         # buildings, > 2 m apart
        add(box((-45 + 18 * b, 18 + (b % 2) * 4, 2), (10, 0.3, 8), n(1500 + 300 * b)), 50)
    add(box((48, -18, 1), (1.5, 0.3, 4), n(200)), 50)                          # too small (min 300)
    for v in range(10):                                                        # vegetation blobs (tol 2, min 200)
        add(box((-40 + 9 * v, -14 - (v % 3) * 5, 0.5), (4, 4, 3), n(150 + 180 * v)), 70)
    for t in range(8):                                                         # trunks: dense vertical lines (tol 0.2, min 50)
        h = np.sort(rng.random(n(40 + 15 * t))) * 3.0 - 1.5
        add(np.stack((np.full_like(h, -40 + 9 * t) + rng.normal(0, 0.01, h.size),
                      np.full_like(h, -11.0) + rng.normal(0, 0.01, h.size), h), axis=1), 71)
    for t in range(5):                                                         # poles (tol 0.2, min 100)
        h = np.sort(rng.random(n(80 + 20 * t))) * 5.0 - 1.5
        add(np.stack((np.full_like(h, -30 + 15 * t) + rng.normal(0, 0.01, h.size),
                      np.full_like(h, 8.2) + rng.normal(0, 0.01, h.size), h), axis=1), 80)
    for t in range(4):                                                         # traffic signs (tol 0.2, min 50)
        add(box((-25 + 15 * t, 8.2, 3.2), (0.6, 0.05, 0.6), n(40 + 15 * t)), 81)
    add(box((0, 12, -0.5), (60, 0.1, 1.2), n(2500)), 51)                       # fence (tol 0.5, min 100)
    add(box((45, 12, -0.5), (3, 0.1, 1.2), n(60)), 51)                         # ... short piece below min size
    add(box((0, -30, -1.5), (100, 12, 0.3), n(9000)), 72)                      # terrain (tol 2, min 300)
    add(box((30, 30, -1.5), (20, 10, 0.3), n(800)), 49)                        # other-ground
    for c in range(6):                                                         # cars with instance ids
        add(box((-35 + 12 * c, 2.0 * (-1) ** c, -0.9), (4, 1.8, 1.5), n(150 + 120 * c)), 10, inst=c + 1)
    add(box((40, 2, -0.9), (4, 1.8, 1.5), 15), 10, inst=9)                     # an instance of <= 20 points: dropped
    add(box((46, -2, -0.9), (4, 1.8, 1.5), n(60)), 10, inst=0)                 # car points without an instance id
    add(box((-20, 26, 0), (8, 2.5, 3), n(900)), 18, inst=1)                    # truck with an instance id
    add(box((10, 27, 0), (10, 2.5, 3), n(700)), 20)                            # other-vehicle WITHOUT instance ids: Euclidean
    add(box((26, 27, 0), (1, 1, 1), n(40)), 20)                                # ... and a fragment below min size 100
    add(box((5, 6, -0.7), (0.5, 0.5, 1.7), n(120)), 30, inst=3)                # person: discarded class
    add(box((0, 0, 5), (120, 80, 1), n(1500)), 0)                              # unlabeled
    add(box((0, 0, 6), (120, 80, 1), n(300)), 1)                               # outlier -> unlabeled
    add(box((-10, 9, -1.2), (1.5, 0.6, 1.0), n(150)), 11, inst=2)              # bicycle: discarded class
    xyz = np.concatenate(pts)
    labels = np.concatenate(lab)
    perm = rng.permutation(len(labels))
    points = np.concatenate((xyz, rng.random((len(labels), 1))), axis=1).astype(np.float32)[perm]
    return np.ascontiguousarray(points), np.ascontiguousarray(labels[perm])


def landmark_world(seed, scans=100, sessions=3, transient_frac=0.15, closures=120, node_num=100, sensor_range=50.0,
                   center_noise=0.15, dropout=0.12, density=0.0062, region=60.0, mix_alpha=3.0, odo_yaw=0.004, odo_t=0.03):
    """One world seen by several drives, with the identity of every node kept: for the landmark map.

    world_sequence's world and rendering (landmarks uniform over the trajectories' bounding box + sensor_range, a label
    mix per region, heights in [-2, 1]; a scan sees the landmarks within sensor_range in its sensor frame, each dropped
    with probability `dropout` and jittered by N(0, center_noise) m, the nearest node_num - 40 kept, listed
    label-ascending), driven `sessions` times along closure_world's trajectory (1 m per scan) with drift_world's jitter
    of N(0, 0.5) m and N(0, 0.03) rad per scan.  A share `transient_frac` of the landmarks exists during ONE drive only
    (a parked car).  The odometry of a drive is integrated from its true relative motions perturbed by N(0, odo_yaw) rad
    and N(0, odo_t) m in a frame of its own (drive d: rotated by 1.1 d rad, shifted by (40 d, -25 d)), as in drift_world.
    True closures join a scan of one drive to a scan within +-2 indices of another drive.
    -> dict: centers f32 [M,N,3], labels i32 [M,N] (M = sessions * scans, -1 = padding); truth, odom f64 [M,4] planar
    poses (c, s, x, y), a scan point into the map frame; starts i32 [sessions]; node_id i32 [M,N], the true landmark of
    every node (-1 = padding); transient_session i32 [landmarks], the one drive a transient exists in (-1 = permanent);
    land_xy f64 [landmarks,2], land_label i32 [landmarks]; rows, cols i32 [closures].  numpy only."""
    rng = np.random.default_rng(seed + 67867967)
    S, D, C = int(scans), int(sessions), int(closures)
    heading, xy = _random_walk(rng, S)
    drives = []
    for d in range(D):
        xyd = xy + rng.normal(0.0, 0.5, size=(S, 2))
        drives.append((heading + rng.normal(0.0, 0.03, size=S), xyd))
    all_xy = np.concatenate([x for _, x in drives])
    lo, hi = all_xy.min(0) - sensor_range, all_xy.max(0) + sensor_range
    n_land = max(int(density * float(np.prod(hi - lo))), 1)
    land_xy = rng.uniform(lo, hi, size=(n_land, 2))
    land_h = rng.uniform(-2.0, 1.0, size=n_land)
    reg = np.floor((land_xy - lo) / region).astype(np.int64)
    nreg = reg.max(0) + 1
    mix = rng.dirichlet(_KITTI_LABEL_P * mix_alpha + 1e-3, size=int(nreg[0] * nreg[1]))
    cum = np.cumsum(mix[reg[:, 0] * nreg[1] + reg[:, 1]], axis=1)
    land_lab = np.minimum((rng.random(n_land)[:, None] > cum).sum(1), NUM_LABELS - 1)
    transient = np.where(rng.random(n_land) < float(transient_frac), rng.integers(0, max(D, 1), size=n_land), -1)
    max_real = max(node_num - 40, 1)
    M = D * S
    centers = np.zeros((M, node_num, 3), dtype=np.float32)
    labels = -np.ones((M, node_num), dtype=np.int32)
    node_id = -np.ones((M, node_num), dtype=np.int32)
    truth, odom = [], []
    for d, (hd, xyd) in enumerate(drives):
        exists = (transient < 0) | (transient == d)
        for t in range(S):
            dl = land_xy - xyd[t]
            r2 = (dl * dl).sum(1)
            seen = np.flatnonzero((r2 <= sensor_range * sensor_range) & exists)
            seen = seen[rng.random(seen.size) >= dropout]
            if seen.size > max_real:
                seen = seen[np.argsort(r2[seen], kind="stable")[:max_real]]
            c, s = np.cos(hd[t]), np.sin(hd[t])
            fwd = dl[seen, 0] * c + dl[seen, 1] * s
            left = -dl[seen, 0] * s + dl[seen, 1] * c
            pts = np.stack([fwd, left, land_h[seen]], axis=1) + rng.normal(0.0, center_noise, size=(seen.size, 3))
            order = np.argsort(land_lab[seen], kind="stable")
            n, g = seen.size, d * S + t
            centers[g, :n] = pts[order]
            labels[g, :n] = land_lab[seen][order]
            node_id[g, :n] = seen[order]
        Xt = _se2(hd, xyd[:, 0], xyd[:, 1])
        rel = _se2_compose(_se2_inverse(Xt[:-1]), Xt[1:])
        rel = _se2_compose(rel, _se2(rng.normal(0.0, odo_yaw, size=S - 1), rng.normal(0.0, odo_t, size=S - 1),
                                     rng.normal(0.0, odo_t, size=S - 1)))
        Xo = np.empty((S, 4), dtype=np.float64)
        Xo[0] = _se2_compose(_se2(1.1 * d, 40.0 * d, -25.0 * d), Xt[0])
        for k in range(S - 1):
            Xo[k + 1] = _se2_compose(Xo[k], rel[k])
        truth.append(Xt)
        odom.append(Xo)
    a = rng.integers(0, D, size=C)
    b = (a + rng.integers(1, max(D, 2), size=C)) % D if D > 1 else a
    i = rng.integers(0, S, size=C)
    j = np.clip(i + rng.integers(-2, 3, size=C), 0, S - 1)
    return {"centers": centers, "labels": labels, "truth": np.concatenate(truth), "odom": np.concatenate(odom),
            "starts": (np.arange(D) * S).astype(np.int32), "node_id": node_id,
            "transient_session": transient.astype(np.int32), "land_xy": land_xy, "land_label": land_lab.astype(np.int32),
            "rows": (a * S + i).astype(np.int32), "cols": (b * S + j).astype(np.int32)}
