"""NumPy reference of the incremental update of a landmark map (include/sgpr_landmark_update.h, sgpr_landmark_update;
DESIGN.md §32): the header's definition in float64, one rounding per operation (NumPy rounds every ufunc on its own),
integer sums.  Map points, links, components and the record of a new landmark are landmark_ref's: the new nodes go
through landmark_ref.landmark_map on a masked label array, as the device runs sgpr_landmark_map's kernels on one.

update(...) returns a dict with every output of the call.  update(..., mutant=NAME) is the definition with one rule
altered (MUTANTS): what a subtly wrong kernel would compute; tests/test_landmark_update_host.py proves that each one
changes an output on some case."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_ref  # noqa: E402

FIX = landmark_ref.FIX            # 2^24
LIMIT = landmark_ref.LIMIT        # 2^37
D2_CAP = landmark_ref.D2_CAP      # 2^20
MAX_COUNT = 262144                # 2^18
SUM_LIMIT = 274877906944.0        # 2^38
RECORD = ("center", "label", "count", "first", "sessions", "spread")

# "no_parallel_axis": v = spread spread, the old members' distances as if the centre had not moved; "old_centre": d2 of
# the observations about the OLD centre; "float_sum": center' by a float64 sum (center n0 + the map points in node order)
# / count'; "ids_high": new landmarks numbered by their HIGHEST member; "first_no_base": first of a new landmark without
# node_base; "session_no_base": session bits without session_base; "recompute_unobserved": a record without an
# observation goes through the formulas with n1 = 0 instead of being copied; "new_links_obs": a new node that links (the
# LINK rule) to an observation becomes an observation of that node's landmark (of the lowest such node)
MUTANTS = ("no_parallel_axis", "old_centre", "float_sum", "ids_high", "first_no_base", "session_no_base", "recompute_unobserved",
           "new_links_obs")


def workspace_bytes(Q, N, L):
    """sgpr_landmark_update_workspace_bytes: sgpr_landmark_map's workspace for the Q N nodes, two int32 per node, 52
    bytes of accumulators and centre per old landmark, two blocks of counters"""
    P = int(Q) * int(N)
    if Q < 0 or N < 0 or L < 0 or P == 0 or P > (1 << 30):
        return 0

    def al(v):
        return (v + 255) & ~255
    return landmark_ref.workspace_bytes(Q, N) + 2 * al(P * 4) + 2 * al(L * 24) + 2 * al(L * 8) + al(L * 4) + 2 * 256


def _table(radius, n_labels):
    radius = np.atleast_1d(np.asarray(radius, np.float64))
    if n_labels is None:
        n_labels = radius.size if radius.size > 1 else 12
    if radius.size == 1:
        radius = np.full(n_labels, radius[0])
    return radius, n_labels


def eligible(lm, radius):
    """ELIGIBLE of every landmark -> bool [L]"""
    c = np.asarray(lm["center"], np.float64).reshape(-1, 3)
    lab = np.asarray(lm["label"], np.int64).reshape(-1)
    cnt = np.asarray(lm["count"], np.int64).reshape(-1)
    sp = np.asarray(lm["spread"], np.float64).reshape(-1)
    ok = (lab >= 0) & (lab < radius.size)
    ok[ok] = radius[lab[ok]] > 0
    ok &= (cnt >= 1) & (cnt <= MAX_COUNT)
    with np.errstate(all="ignore"):
        ok &= np.isfinite(c).all(1) & (np.abs(c * cnt.astype(np.float64)[:, None]) <= SUM_LIMIT).all(1)
        ok &= np.isfinite(sp) & (sp >= 0)
    return ok


def update(centers, labels, poses, assoc, lm, starts=None, session_base=0, node_base=0, radius=0.75, tau_z=0.75, n_labels=None,
           max_landmarks=None, mutant=None):
    """centers f32 [Q,N,3], labels i32 [Q,N], poses f64 [Q,4], assoc i32 [Q,N]; lm: dict of center f64 [L,3], label, count,
    first i32 [L], sessions u64 [L], spread f64 [L] -> dict: the six records of the updated map, L'' = min(L',
    max_landmarks) rows (None: L'), node_landmark i32 [Q,N], num = (L', live, observations, new nodes)"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    lab2 = np.asarray(labels, np.int32)
    Q, N = lab2.shape
    P = Q * N
    radius, n_labels = _table(radius, n_labels)
    tau_z = np.float64(tau_z)
    poses = np.asarray(poses, np.float64).reshape(Q, 4)
    cen = np.asarray(centers, np.float32).reshape(Q, N, 3)
    old = {"center": np.array(np.asarray(lm["center"], np.float64).reshape(-1, 3)), "label": np.array(lm["label"], np.int32).reshape(-1),
           "count": np.array(lm["count"], np.int32).reshape(-1), "first": np.array(lm["first"], np.int32).reshape(-1),
           "sessions": np.array(lm["sessions"]).astype(np.uint64).reshape(-1), "spread": np.array(lm["spread"], np.float64).reshape(-1)}
    L = old["label"].size
    m = landmark_ref.map_points(cen, poses).reshape(P, 3)
    lab = lab2.reshape(P).astype(np.int64)
    live = (lab >= 0) & (lab < n_labels)
    live[live] = radius[lab[live]] > 0
    live &= np.repeat(np.isfinite(poses).all(1), N)
    with np.errstate(all="ignore"):
        live &= np.isfinite(m).all(1) & (np.abs(m) <= LIMIT).all(1)
    a = np.array(assoc, np.int64).reshape(P)
    elig = eligible(old, radius)
    inside = live & (a >= 0) & (a < L)
    seen = inside.copy()
    seen[inside] = elig[a[inside]] & (old["label"][a[inside]] == lab[inside])
    new = live & (a == -2)
    if mutant == "new_links_obs":
        x, y = landmark_ref._links(m, lab, seen | new, radius, tau_z, None)        # x > y
        for hi, lo in sorted(zip(np.concatenate((x, y)).tolist(), np.concatenate((y, x)).tolist()), key=lambda t: (t[0], -t[1])):
            if new[hi] and seen[lo] and a[lo] >= 0 and (old["label"][a[lo]] == lab[hi]):
                a[hi] = a[lo]                                     # (descending lo: the lowest observation is kept)
        seen = seen | (new & (a >= 0))
        new = new & (a == -2)
    sess = landmark_ref.session_of(Q, starts)[np.arange(P) // max(N, 1)].astype(np.uint64)
    shift = np.uint64(0 if mutant == "session_no_base" else session_base)

    out = {k: v.copy() for k, v in old.items()}
    obs = np.flatnonzero(seen)
    ids = a[obs]
    n1 = np.bincount(ids, minlength=L).astype(np.int64)
    hit = np.flatnonzero((n1 > 0) | (elig if mutant == "recompute_unobserved" else False))
    if hit.size:
        n0 = old["count"][hit].astype(np.float64)
        cnt = old["count"][hit].astype(np.int64) + n1[hit]
        slot = np.full(L, -1, np.int64)
        slot[hit] = np.arange(hit.size)
        row = slot[ids]
        with np.errstate(all="ignore"):
            S = np.rint((old["center"][hit] * n0[:, None]) * FIX).astype(np.int64)
            np.add.at(S, row, np.rint(m[obs] * FIX).astype(np.int64))            # (wraps modulo 2^64 like the device's sums)
            centre = S.astype(np.float64) / (cnt.astype(np.float64) * FIX)[:, None]
            if mutant == "float_sum":
                acc = old["center"][hit] * n0[:, None]
                for r, v in zip(row, m[obs]):
                    acc[r] = acc[r] + v
                centre = acc / cnt.astype(np.float64)[:, None]
            ax, ay = old["center"][hit, 0] - centre[:, 0], old["center"][hit, 1] - centre[:, 1]
            sp = old["spread"][hit]
            v = sp * sp if mutant == "no_parallel_axis" else sp * sp + (ax * ax + ay * ay)
            Qs = np.rint((np.minimum(v, D2_CAP) * n0) * FIX).astype(np.uint64)
            about = old["center"][hit] if mutant == "old_centre" else centre
            ex, ey = m[obs, 0] - about[row, 0], m[obs, 1] - about[row, 1]
            d2 = ex * ex + ey * ey
            np.add.at(Qs, row, np.rint(np.minimum(d2, D2_CAP) * FIX).astype(np.uint64))
            spread = np.sqrt(Qs.astype(np.float64) / (cnt.astype(np.float64) * FIX))
        bits = np.zeros(hit.size, np.uint64)
        np.bitwise_or.at(bits, row, np.uint64(1) << (shift + sess[obs]))
        out["center"][hit] = centre
        out["count"][hit] = cnt.astype(np.int32)
        out["sessions"][hit] = old["sessions"][hit] | bits
        out["spread"][hit] = spread

    # the new landmarks: sgpr_landmark_map on the masked labels, numbered from L
    masked = np.where(new, lab, -1).astype(np.int32).reshape(Q, N)
    fresh = landmark_ref.landmark_map(cen, masked, poses, starts=starts, radius=radius, tau_z=tau_z, n_labels=n_labels,
                                      mutant="ids_high" if mutant == "ids_high" else None)
    n_new = int(fresh["num"][0])
    fresh["first"] = (fresh["first"].astype(np.int64) + (0 if mutant == "first_no_base" else node_base)).astype(np.int32)
    fresh["sessions"] = fresh["sessions"] << shift
    node = np.where(fresh["node_landmark"].reshape(P) >= 0, fresh["node_landmark"].reshape(P) + L, -1).astype(np.int32)
    node[obs] = ids
    total = L + n_new
    k = total if max_landmarks is None else min(total, int(max_landmarks))
    res = {key: np.concatenate((out[key], fresh[key].astype(out[key].dtype)))[:k] for key in RECORD}
    res["node_landmark"] = node.reshape(Q, N)
    res["num"] = np.array([total, int(live.sum()), obs.size, int(new.sum())], np.int32)
    return res


def make_case(Q, N, L, seed, noise=0.1, perturb=0.02, labels=3, radius=0.75, tau_z=0.75):
    """A map of L landmarks of `labels` labels over a square with made-up records (counts 1..9, spreads up to 0.3 m,
    sessions among the first two) and Q scans of N nodes that observe them from slightly perturbed poses; one node in
    twenty is padding, one in twenty an object the map does not hold (some of those in pairs, to link); the association
    is landmark_align_ref's with iters=0 against every landmark.
    -> (centers, labels, poses, assoc, lm dict)"""
    import landmark_align_ref
    rng = np.random.default_rng(seed)
    extent = max(4.0, 1.5 * np.sqrt(max(L, 1)))
    Lp = max(L, 1)
    pts = np.concatenate((rng.uniform(-extent, extent, size=(Lp, 2)), rng.uniform(-1.0, 1.0, size=(Lp, 1))), axis=1)
    lm_label = rng.integers(0, labels, size=Lp)
    ids = rng.integers(0, Lp, size=(Q, N))
    yaw = rng.uniform(-3.0, 3.0, size=Q)
    t = rng.uniform(-5.0, 5.0, size=(Q, 2))
    d = pts[ids][..., :2] + rng.normal(0.0, noise, size=(Q, N, 2))
    new = rng.random((Q, N)) < 0.05
    spots = rng.uniform(-extent, extent, size=(max(Q * N // 40, 1), 2))            # fewer spots than new nodes: some link
    fresh = spots[rng.integers(0, spots.shape[0], size=(Q, N))] + rng.normal(0.0, noise, size=(Q, N, 2))
    d = np.where(new[..., None], fresh, d) - t[:, None, :]
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    centers = np.stack((c * d[..., 0] + s * d[..., 1], c * d[..., 1] - s * d[..., 0],
                        pts[ids][..., 2] + rng.uniform(-0.5, 0.5, size=(Q, N))), axis=-1).astype(np.float32)
    yaw = yaw + rng.normal(0.0, 0.05 * perturb, size=Q)
    t = t + rng.normal(0.0, perturb, size=(Q, 2))
    poses = np.stack((np.cos(yaw), np.sin(yaw), t[:, 0], t[:, 1]), axis=1)
    lab = np.where(rng.random((Q, N)) < 0.05, -1, lm_label[ids]).astype(np.int32)
    lm = {"center": pts[:L].copy(), "label": lm_label[:L].astype(np.int32), "count": rng.integers(1, 10, size=Lp)[:L].astype(np.int32),
          "first": np.sort(rng.choice(max(4 * Lp, 8), size=Lp, replace=False))[:L].astype(np.int32),
          "sessions": rng.integers(1, 4, size=Lp)[:L].astype(np.uint64), "spread": rng.uniform(0.0, 0.3, size=Lp)[:L]}
    assoc = landmark_align_ref.align(centers, lab, poses, lm["center"], lm["label"], radius=radius, tau_z=tau_z, iters=0,
                                     n_labels=12)["node_landmark"]
    return centers, lab, poses, assoc, lm
