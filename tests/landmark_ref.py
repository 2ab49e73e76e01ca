"""NumPy reference of the semantic landmark map (include/sgpr_landmarks.h, sgpr_landmark_map): the
header's definition in float64, one rounding per operation (NumPy rounds every ufunc on its own, there is no fused
multiply-add anywhere), integer sums, and a plain union-find (hook the larger root under the smaller, compress) so that
it needs nothing outside NumPy.

landmark_map(...) returns a dict with every output of the call.  landmark_map(..., mutant=NAME) is the definition with
one rule altered (MUTANTS): what a subtly wrong kernel would compute; tests/test_landmark_host.py proves that each one
changes an output on some case."""
import numpy as np

MAX_LABELS = 64
SESSION_MAX = 64
FIX = 16777216.0            # 2^24
LIMIT = 137438953472.0      # 2^37
D2_CAP = 1048576.0          # 2^20
THREADS = 256
_PAIR_CHUNK = 1 << 22

# "strict": d2 < r r; "dist3d": dz dz joins the distance; "fused_map": c x - s y with one rounding; "float_sum": centres
# by a sequential float64 sum in member order; "ids_high": landmarks numbered by their HIGHEST member; "z_strict"
MUTANTS = ("strict", "dist3d", "fused_map", "float_sum", "ids_high", "z_strict")


def workspace_bytes(G, N):
    """sgpr_landmark_workspace_bytes"""
    P = int(G) * int(N)
    if G < 0 or N < 0 or P == 0 or P > 0x7fffffff:
        return 0
    H = 1024
    while H < 2 * P:
        H <<= 1
    B = (P + THREADS - 1) // THREADS

    def al(v):
        return (v + 255) & ~255
    return al(P * 24) * 2 + al(P * 4) * 5 + al(P * 8) * 2 + al(H * 8) + al(H * 4) + al(B * 4) * 2


def _fused(c, x, z):
    """c x + z as a fused multiply-add would give it (mutant fused_map): x is a widened float32, so with c split at 26
    bits both partial products are exact and the rounding error of fl(c x) is known; it is added back after the sum (one
    rounding up to a double rounding nobody relies on)."""
    hi = (c * 134217729.0) - ((c * 134217729.0) - c)             # Veltkamp: the upper 26 bits of c
    p = c * x
    err = ((hi * x) - p) + ((c - hi) * x)
    s = p + z
    t = s - p
    return s + (((p - (s - t)) + (z - t)) + err)


def map_points(centers, poses, mutant=None):
    """the map point of every node -> float64 [G,N,3]"""
    c = np.asarray(centers, np.float32).astype(np.float64)
    X = np.asarray(poses, np.float64).reshape(-1, 4)[:, None, :]
    x, y = c[..., 0], c[..., 1]
    with np.errstate(all="ignore"):
        if mutant == "fused_map":
            a = _fused(X[..., 0], x, -(X[..., 1] * y))
            b = _fused(X[..., 1], x, X[..., 0] * y)
        else:
            a = X[..., 0] * x - X[..., 1] * y
            b = X[..., 1] * x + X[..., 0] * y
        return np.stack((a + X[..., 2], b + X[..., 3], c[..., 2]), axis=-1)


def session_of(G, starts):
    """session(g) of every scan: the largest j with starts[j] <= g"""
    if starts is None:
        return np.zeros(G, np.int64)
    return np.searchsorted(np.asarray(starts, np.int64), np.arange(G), side="right") - 1


def _links(m, lab, live, radius, tau_z, mutant):
    """every linked pair (a, b), a > b, of flat node indices"""
    out_a, out_b = [], []
    for l in np.unique(lab[live]):
        r = float(radius[l])
        idx = np.flatnonzero(live & (lab == l))
        idx = idx[np.argsort(m[idx, 0], kind="stable")]
        xs = m[idx, 0]
        # candidates: everything within a window a little wider than r along x (a superset of the rule)
        reach = r * 1.000001 + 1e-300
        # (... and by more than the rounding of the subtraction at the far end of the coordinate range)
        lo = (np.searchsorted(xs, xs - (reach + np.abs(xs) * 1e-15), side="left") if np.isfinite(reach)
              else np.zeros(idx.size, np.int64))
        cnt = np.arange(idx.size) - lo
        pos = 0
        while pos < idx.size:
            end = pos + 1
            tot = int(cnt[pos])
            while end < idx.size and tot + cnt[end] <= _PAIR_CHUNK:
                tot += int(cnt[end])
                end += 1
            i = np.repeat(np.arange(pos, end), cnt[pos:end])
            off = np.arange(tot) - np.repeat(np.cumsum(cnt[pos:end]) - cnt[pos:end], cnt[pos:end])
            j = np.repeat(lo[pos:end], cnt[pos:end]) + off
            a, b = idx[i], idx[j]
            with np.errstate(all="ignore"):
                dx, dy = m[a, 0] - m[b, 0], m[a, 1] - m[b, 1]
                d2 = dx * dx + dy * dy
                dz = np.abs(m[a, 2] - m[b, 2])
                if mutant == "dist3d":
                    d2 = d2 + dz * dz
                r2 = np.float64(r) * np.float64(r)
                ok = (d2 < r2) if mutant == "strict" else (d2 <= r2)
                ok &= (dz < tau_z) if mutant == "z_strict" else (dz <= tau_z)
            out_a.append(a[ok])
            out_b.append(b[ok])
            pos = end
    if not out_a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_a), np.concatenate(out_b)


def _components(P, a, b):
    """union-find over the links: the larger root is hooked under the smaller, then every path is compressed; the root
    of a component is its lowest member -> parent [P]"""
    parent = np.arange(P, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            return parent
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up


def landmark_map(centers, labels, poses, starts=None, radius=0.75, tau_z=0.75, n_labels=None, max_landmarks=None,
                 mutant=None):
    """centers f32 [G,N,3], labels i32 [G,N], poses f64 [G,4] -> dict: center f64 [L',3], label, count, first i32 [L'],
    sessions u64 [L'], spread f64 [L'] with L' = min(L, max_landmarks) (None: L), node_landmark i32 [G,N],
    num = (L, live nodes), links (the number of linked pairs)."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    lab2 = np.asarray(labels, np.int32)
    G, N = lab2.shape
    P = G * N
    radius = np.atleast_1d(np.asarray(radius, np.float64))
    if n_labels is None:
        n_labels = radius.size if radius.size > 1 else 12
    if radius.size == 1:
        radius = np.full(n_labels, radius[0])
    poses = np.asarray(poses, np.float64).reshape(G, 4)
    m = map_points(np.asarray(centers, np.float32).reshape(G, N, 3), poses, mutant).reshape(P, 3)
    lab = lab2.reshape(P).astype(np.int64)
    live = (lab >= 0) & (lab < n_labels)
    live[live] = radius[lab[live]] > 0
    live &= np.repeat(np.isfinite(poses).all(1), N)
    with np.errstate(all="ignore"):
        live &= np.isfinite(m).all(1) & (np.abs(m) <= LIMIT).all(1)
    a, b = _links(m, lab, live, radius, np.float64(tau_z), mutant)
    parent = _components(P, a, b)
    members = np.flatnonzero(live)
    root = parent[members]
    if mutant == "ids_high":                                     # numbered by the highest member
        top = np.zeros(P, np.int64)
        np.maximum.at(top, root, members)
        keys, lid = np.unique(top[root], return_inverse=True)
    else:
        keys, lid = np.unique(root, return_inverse=True)         # roots ascending: ids by the lowest member
    L = keys.size
    node_landmark = np.full(P, -1, np.int32)
    node_landmark[members] = lid
    count = np.bincount(lid, minlength=L).astype(np.int64)
    first = np.full(L, P, np.int64)
    np.minimum.at(first, lid, members)
    label = np.zeros(L, np.int32)
    label[lid] = lab[members]
    sessions = np.zeros(L, np.uint64)
    np.bitwise_or.at(sessions, lid, np.uint64(1) << session_of(G, starts)[members // N].astype(np.uint64))
    mm = m[members]
    S = np.zeros((L, 3), np.int64)
    with np.errstate(all="ignore"):
        np.add.at(S, lid, np.rint(mm * FIX).astype(np.int64))   # (wraps modulo 2^64 like the device's sums)
        center = S.astype(np.float64) / (count.astype(np.float64) * FIX)[:, None]
        if mutant == "float_sum":
            center = np.zeros((L, 3))
            for i, v in zip(lid, mm):
                center[i] = center[i] + v
            center = center / count.astype(np.float64)[:, None]
        ex, ey = mm[:, 0] - center[lid, 0], mm[:, 1] - center[lid, 1]
        d2 = ex * ex + ey * ey
        Q = np.zeros(L, np.uint64)
        np.add.at(Q, lid, np.rint(np.minimum(d2, D2_CAP) * FIX).astype(np.uint64))
        spread = np.sqrt(Q.astype(np.float64) / (count.astype(np.float64) * FIX))
    k = L if max_landmarks is None else min(L, int(max_landmarks))
    return {"center": center[:k], "label": label[:k], "count": count[:k].astype(np.int32), "first": first[:k].astype(np.int32),
            "sessions": sessions[:k], "spread": spread[:k], "node_landmark": node_landmark.reshape(G, N),
            "num": np.array([L, members.size], np.int32), "links": int(a.size)}


def virtual_scans(center, label, poses, sensor_range=50.0, node_num=100, keep=None):
    """landmarks.virtual_scans, query by query: the kept landmarks within sensor_range (planar) of every pose in its
    sensor frame, nearest first up to node_num (ties to the lower id), listed label-ascending (stable), padded with
    centre 0 / label -1 -> (centers f32 [Q,node_num,3], labels i32 [Q,node_num])"""
    center = np.asarray(center, np.float64).reshape(-1, 3)
    label = np.asarray(label, np.int64).reshape(-1)
    if keep is not None:
        center, label = center[np.asarray(keep, bool)], label[np.asarray(keep, bool)]
    poses = np.asarray(poses, np.float64).reshape(-1, 4)
    out_c = np.zeros((poses.shape[0], node_num, 3), np.float32)
    out_l = -np.ones((poses.shape[0], node_num), np.int32)
    for i, (c, s, X, Y) in enumerate(poses):
        dx, dy = center[:, 0] - X, center[:, 1] - Y
        d2 = dx * dx + dy * dy
        seen = np.flatnonzero(d2 <= sensor_range * sensor_range)
        seen = seen[np.argsort(d2[seen], kind="stable")[:node_num]]
        seen = seen[np.argsort(label[seen], kind="stable")]
        n = seen.size
        out_c[i, :n] = np.stack((c * dx[seen] + s * dy[seen], c * dy[seen] - s * dx[seen], center[seen, 2]), axis=1)
        out_l[i, :n] = label[seen]
    return out_c, out_l
