"""NumPy reference of the visibility tallies of a landmark map (include/sgpr_landmark_persist.h, sgpr_landmark_persist;
DESIGN.md §33): the header's definition in float64, one rounding per operation (NumPy rounds every ufunc on its own), the
view test against EVERY landmark and the observations as the set of distinct (scan, landmark) pairs.  Map points, the live
rule and the eligible rule are landmark_ref's and landmark_align_ref's.

persist(...) returns a dict with every output of the call.  persist(..., mutant=NAME) is the definition with one rule
altered (MUTANTS): what a subtly wrong kernel would compute; tests/test_landmark_persist_host.py proves that each one
changes an output on some case."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref  # noqa: E402
import landmark_ref  # noqa: E402

LIMIT = landmark_align_ref.LIMIT      # 2^37
NONFINITE = 1
OUTPUTS = ("expected", "seen", "keep", "scan_stat", "view", "num")
_CHUNK = 1 << 22                      # entries of the largest scan x landmark matrix alive

# "count_nodes": every observing node counts, not every scan; "view_map_frame": far2 from the MAP point of the nodes;
# "no_margin": v = min(max_range, far); "view_strict": d2 < v v at the view edge; "decide_le": retired at
# seen <= ratio expected; "beyond_view_dropped": an observed landmark that is not in view is not expected;
# "label_unchecked": an association with a landmark of another label observes it; "use_ignored": d_lm_use is not read
MUTANTS = ("count_nodes", "view_map_frame", "no_margin", "view_strict", "decide_le", "beyond_view_dropped", "label_unchecked",
           "use_ignored")


def workspace_bytes(Q, N, L):
    """sgpr_landmark_persist_workspace_bytes: three int32 per landmark (label, slot, item), a table of H slots with a
    key and two int32 each, one block of counters"""
    if Q < 0 or N < 0 or L < 0 or Q * N == 0 or Q * N > 0x7fffffff:
        return 0
    H = 1024
    while H < 2 * L:
        H <<= 1

    def al(v):
        return (v + 255) & ~255
    return 3 * al(L * 4) + al(H * 8) + 2 * al(H * 4) + 256


def persist(centers, labels, poses, assoc, lm, radius=0.75, n_labels=None, max_range=50.0, margin=2.0, min_expected=5,
            max_seen_ratio=0.3, mutant=None):
    """centers f32 [Q,N,3], labels i32 [Q,N], poses f64 [Q,4], assoc i32 [Q,N]; lm: dict of center f64 [L,3], label i32 [L]
    and, optionally, use u8 [L] (absent or None: every landmark takes part) -> dict: expected, seen i32 [L], keep u8 [L],
    scan_stat i32 [Q,4], view f64 [Q], num i32 [4]"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    lab2 = np.asarray(labels, np.int32)
    Q, N = lab2.shape
    radius = np.atleast_1d(np.asarray(radius, np.float64))
    if n_labels is None:
        n_labels = radius.size if radius.size > 1 else 12
    if radius.size == 1:
        radius = np.full(n_labels, radius[0])
    max_range, margin, ratio = np.float64(max_range), np.float64(margin), np.float64(max_seen_ratio)
    cen = np.asarray(centers, np.float32).reshape(Q, N, 3)
    X = np.asarray(poses, np.float64).reshape(Q, 4)
    c = np.asarray(lm["center"], np.float64).reshape(-1, 3)
    lm_label = np.asarray(lm["label"], np.int64).reshape(-1)
    L = lm_label.size
    use = None if mutant == "use_ignored" else lm.get("use")
    elab = landmark_align_ref.eligible(c, lm_label, use, radius)
    elig = elab >= 0

    # live nodes and the view range
    m = landmark_ref.map_points(cen, X)
    lab = lab2.astype(np.int64)
    finite = np.isfinite(X).all(1)
    live = (lab >= 0) & (lab < n_labels)
    live[live] = radius[lab[live]] > 0
    with np.errstate(all="ignore"):
        live &= finite[:, None] & np.isfinite(m).all(2) & (np.abs(m) <= LIMIT).all(2)
        if mutant == "view_map_frame":
            x, y = m[..., 0], m[..., 1]
        else:
            x, y = cen[..., 0].astype(np.float64), cen[..., 1].astype(np.float64)
        far2 = np.where(live, x * x + y * y, 0.0).max(axis=1, initial=0.0)
        v = np.minimum(max_range, np.sqrt(far2))
        if mutant != "no_margin":
            v = v - margin
        v2 = v * v
    has_view = v > 0

    # the observations: distinct (scan, landmark) pairs
    a = np.asarray(assoc, np.int64).reshape(Q, N)
    valid = live & (a >= 0) & (a < L)
    qi = np.broadcast_to(np.arange(Q)[:, None], (Q, N))
    if L:
        hit = elab[a[valid]]
        valid[valid] = (hit >= 0) if mutant == "label_unchecked" else (hit == lab[valid])
    pairs, nodes = np.unique(qi[valid] * max(L, 1) + a[valid], return_counts=True)
    pq, pl = pairs // max(L, 1), pairs % max(L, 1)
    pair_in_view = np.zeros(pairs.size, bool)

    expected = np.zeros(L, np.int64)
    scan_exp = np.zeros(Q, np.int64)
    step = max(1, _CHUNK // max(L, 1))
    for lo in range(0, Q, step):
        hi = min(lo + step, Q)
        with np.errstate(all="ignore"):
            dx = c[None, :, 0] - X[lo:hi, None, 2]
            dy = c[None, :, 1] - X[lo:hi, None, 3]
            d2 = dx * dx + dy * dy
            near = (d2 < v2[lo:hi, None]) if mutant == "view_strict" else (d2 <= v2[lo:hi, None])
        view = near & has_view[lo:hi, None] & elig[None, :]
        expected += view.sum(0)
        scan_exp[lo:hi] = view.sum(1)
        sel = (pq >= lo) & (pq < hi)
        pair_in_view[sel] = view[pq[sel] - lo, pl[sel]]
    seen = np.bincount(pl, minlength=L).astype(np.int64)
    scan_seen = np.bincount(pq, minlength=Q).astype(np.int64)
    if mutant != "beyond_view_dropped":
        out = ~pair_in_view
        expected += np.bincount(pl[out], minlength=L)
        scan_exp += np.bincount(pq[out], minlength=Q)
    if mutant == "count_nodes":
        extra = np.bincount(pl, weights=nodes - 1, minlength=L).astype(np.int64)
        seen, expected = seen + extra, expected + extra

    enough = elig & (expected >= int(min_expected))
    with np.errstate(all="ignore"):
        bar = ratio * expected.astype(np.float64)
    few = (seen.astype(np.float64) <= bar) if mutant == "decide_le" else (seen.astype(np.float64) < bar)
    retire = enough & few
    stat = np.stack((scan_exp, scan_seen, live.sum(1), np.where(finite, 0, NONFINITE)), axis=1).astype(np.int32)
    return {"expected": expected.astype(np.int32), "seen": seen.astype(np.int32), "keep": (~retire).astype(np.uint8),
            "scan_stat": stat.reshape(Q, 4), "view": v, "num": np.array([retire.sum(), enough.sum(), elig.sum(), has_view.sum()], np.int32)}


def make_case(Q, N, L, seed, labels=3, noise=0.1, gone=0.2, spread=None, specials=True):
    """A map of L landmarks of `labels` labels over a square (half side `spread`; None: grown with L) and Q scans of N
    slots from poses inside it.  A scan renders the landmarks within a range of its own, nearest first, each with
    probability 0.8 - a share `gone` of the landmarks is never rendered - and fills the slots left over with second nodes
    on rendered landmarks and with padding; a few nodes carry no label or another label; the slots are shuffled.  One
    landmark in ten is masked out, a few are ineligible.  The association is landmark_align_ref's with iters=0 against
    EVERY landmark, then a few nodes are put on a far landmark, most of them on one of their label, and a few get values outside the map.
    specials: scan 1 has a pose that is not finite (Q >= 3), scan 2 nothing but padding (Q >= 5).
    -> (centers, labels, poses, assoc, lm dict with center, label, use)"""
    rng = np.random.default_rng(seed)
    Lp = max(L, 1)
    extent = max(6.0, 2.0 * np.sqrt(Lp)) if spread is None else float(spread)
    pts = np.concatenate((rng.uniform(-extent, extent, size=(Lp, 2)), rng.uniform(-1.0, 1.0, size=(Lp, 1))), axis=1)
    lm_label = rng.integers(0, labels, size=Lp)
    is_gone = rng.random(Lp) < gone
    yaw = rng.uniform(-3.0, 3.0, size=Q)
    t = rng.uniform(-0.5 * extent, 0.5 * extent, size=(Q, 2))
    reach = rng.uniform(0.4, 1.0, size=Q) * extent
    centers = np.zeros((Q, N, 3), np.float32)
    lab = np.full((Q, N), -1, np.int32)
    for q in range(Q):
        d = pts[:, :2] - t[q]
        r2 = (d * d).sum(1)
        shown = np.flatnonzero((r2 <= reach[q] * reach[q]) & ~is_gone & (rng.random(Lp) < 0.8))[:L]
        shown = shown[np.argsort(r2[shown], kind="stable")][:N]
        ids = shown
        if shown.size and shown.size < N:
            more = rng.integers(0, shown.size, size=N - shown.size)
            ids = np.concatenate((shown, shown[more[rng.random(more.size) < 0.7]]))
        k = ids.size
        if k == 0:
            continue
        p = pts[ids] + np.concatenate((rng.normal(0.0, noise, size=(k, 2)), rng.uniform(-0.3, 0.3, size=(k, 1))), axis=1)
        e = p[:, :2] - t[q]
        co, si = np.cos(yaw[q]), np.sin(yaw[q])
        slots = rng.permutation(N)[:k]
        centers[q, slots] = np.stack((co * e[:, 0] + si * e[:, 1], co * e[:, 1] - si * e[:, 0], p[:, 2]), axis=1).astype(np.float32)
        nl = lm_label[ids].copy()
        roll = rng.random(k)
        nl = np.where(roll < 0.05, -1, np.where(roll < 0.09, (nl + 1) % labels, nl))
        lab[q, slots] = nl
    poses = np.stack((np.cos(yaw), np.sin(yaw), t[:, 0], t[:, 1]), axis=1)
    if specials and Q >= 3:
        poses[1, 2] = np.nan
    if specials and Q >= 5:
        lab[2] = -1
    use = (rng.random(Lp) >= 0.1).astype(np.uint8)
    lm_label = np.where(rng.random(Lp) < 0.03, -1, lm_label)
    if L >= 20:
        pts[7, 1] = np.nan
        pts[11, 0] = 1e12                                    # past 2^37
    lm = {"center": pts[:L].copy(), "label": lm_label[:L].astype(np.int32), "use": use[:L].copy()}
    assoc = landmark_align_ref.align(centers, lab, poses, lm["center"], lm["label"], radius=0.75, tau_z=0.75, iters=0,
                                     n_labels=12)["node_landmark"].astype(np.int32)
    if L:
        far = (rng.random((Q, N)) < 0.03) & (lab >= 0)
        for q, n in zip(*np.nonzero(far)):
            same = np.flatnonzero(lm["label"] == lab[q, n]) if rng.random() < 0.6 else np.arange(L)     # (or of any label)
            if same.size:
                assoc[q, n] = same[rng.integers(0, same.size)]
    odd = rng.random((Q, N)) < 0.02
    assoc[odd] = rng.choice(np.array([-3, L, L + 5, 2 ** 31 - 1, -2 ** 31], np.int64), size=int(odd.sum())).astype(np.int32)
    return centers, lab, poses, assoc, lm
