"""NumPy reference of the alignment of scans to a landmark map (include/sgpr_landmark_align.h, sgpr_landmark_align;
DESIGN.md §31): the header's definition in float64, one rounding per operation (NumPy rounds every ufunc on its own), the
match by a dense search over all landmarks ordered by (d2, id), the scan sums W as 64 partials and the halving tree
(landmark_refine_ref.scan_sum: the same W), exactly as defined.

align(...) returns a dict with every output of the call.  align(..., mutant=NAME) is the definition with one rule altered
(MUTANTS): what a subtly wrong kernel would compute; tests/test_landmark_align_host.py proves that each one changes an
output on some case."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_ref  # noqa: E402
from landmark_refine_ref import scan_sum  # noqa: E402

LIMIT = 137438953472.0      # 2^37
NONFINITE, KEPT = 1, 2
QNAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]
_CHUNK = 1 << 22            # entries of the largest distance matrix alive

# "ties_high": equal d2 goes to the HIGHEST id; "dist3d": dz dz joins the distance of the gate and of the order;
# "sequential": the scan sums in slot order instead of W; "uncentred": the moments of p, l instead of p', l';
# "fused_map": c x - s y with one rounding
MUTANTS = ("ties_high", "dist3d", "sequential", "uncentred", "fused_map")


def workspace_bytes(Q, N, L):
    """sgpr_landmark_align_workspace_bytes"""
    if Q < 0 or N < 0 or L < 0 or Q * N == 0 or Q * N > 0x7fffffff:
        return 0
    H = 1024
    while H < 2 * L:
        H <<= 1

    def al(v):
        return (v + 255) & ~255
    return 2 * al(L * 4) + al(H * 8) + al(H * 4)


def eligible(lm_center, lm_label, lm_use, radius):
    """the label of every eligible landmark, -1 of any other -> int64 [L]"""
    c = np.asarray(lm_center, np.float64).reshape(-1, 3)
    lab = np.asarray(lm_label, np.int64).reshape(-1)
    ok = (lab >= 0) & (lab < radius.size)
    ok[ok] = radius[lab[ok]] > 0
    if lm_use is not None:
        ok &= np.asarray(lm_use).reshape(-1) != 0
    with np.errstate(all="ignore"):
        ok &= np.isfinite(c).all(1) & (np.abs(c) <= LIMIT).all(1)
    return np.where(ok, lab, -1)


def match(m, lab, live, c, elab, radius, tau_z, mutant=None):
    """the match of every node: m [P,3] map points, lab [P], live [P]; c [L,3], elab [L] -> (id int64 [P]: the landmark,
    -2 live without one, -1 dead; d2 float64 [P] of the matched)"""
    P = m.shape[0]
    out = np.where(live, -2, -1).astype(np.int64)
    best = np.zeros(P)
    for l in np.unique(lab[live]):
        nodes = np.flatnonzero(live & (lab == l))
        lms = np.flatnonzero(elab == l)                          # ascending ids
        if lms.size == 0:
            continue
        r2 = np.float64(radius[l]) * np.float64(radius[l])
        step = max(1, _CHUNK // lms.size)
        for lo in range(0, nodes.size, step):
            idx = nodes[lo:lo + step]
            with np.errstate(all="ignore"):
                ex = m[idx, 0][:, None] - c[lms, 0][None, :]
                ey = m[idx, 1][:, None] - c[lms, 1][None, :]
                d2 = ex * ex + ey * ey
                dz = np.abs(m[idx, 2][:, None] - c[lms, 2][None, :])
                if mutant == "dist3d":
                    d2 = d2 + dz * dz
                ok = (d2 <= r2) & (dz <= tau_z)
            key = np.where(ok, d2, np.inf)
            if mutant == "ties_high":
                j = key.shape[1] - 1 - np.argmin(key[:, ::-1], axis=1)
            else:
                j = np.argmin(key, axis=1)                       # the first minimum: the lowest id
            rows = np.arange(idx.size)
            hit = ok[rows, j]                  # (points and centres lie within 2^37: d2 <= 2^77 is finite, never the mask)
            out[idx[hit]] = lms[j[hit]]
            best[idx[hit]] = d2[rows, j][hit]
    return out, best


def align(centers, labels, poses, lm_center, lm_label, lm_use=None, radius=0.75, tau_z=0.75, iters=10, min_nodes=6,
          n_labels=None, mutant=None):
    """centers f32 [Q,N,3], labels i32 [Q,N], poses f64 [Q,4]; lm_center f64 [L,3], lm_label i32 [L], lm_use u8 [L] or
    None -> dict: poses f64 [Q,4], node_landmark i32 [Q,N], stat i32 [Q,4], rms f64 [Q]"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    lab2 = np.asarray(labels, np.int32)
    Q, N = lab2.shape
    radius = np.atleast_1d(np.asarray(radius, np.float64))
    if n_labels is None:
        n_labels = radius.size if radius.size > 1 else 12
    if radius.size == 1:
        radius = np.full(n_labels, radius[0])
    tau_z = np.float64(tau_z)
    cen = np.asarray(centers, np.float32).reshape(Q, N, 3)
    x, y = cen[..., 0].astype(np.float64), cen[..., 1].astype(np.float64)
    X0 = np.array(np.asarray(poses, np.float64).reshape(Q, 4))
    X = X0.copy()
    c = np.asarray(lm_center, np.float64).reshape(-1, 3)
    elab = eligible(c, lm_label, lm_use, radius)
    finite0 = np.isfinite(X0).all(1)
    lab = lab2.reshape(-1).astype(np.int64)
    lab_ok = (lab >= 0) & (lab < n_labels)
    lab_ok[lab_ok] = radius[lab[lab_ok]] > 0
    T = int(iters)
    steps = np.zeros(Q, np.int64)
    kept = np.zeros(Q, bool)
    for k in range(T + 1):
        m = landmark_ref.map_points(cen, X, "fused_map" if mutant == "fused_map" else None).reshape(-1, 3)
        with np.errstate(all="ignore"):
            live = lab_ok & np.repeat(finite0, N) & np.isfinite(m).all(1) & (np.abs(m) <= LIMIT).all(1)
        ids, d2 = match(m, lab, live, c, elab, radius, tau_z, mutant)
        ids, d2, live2 = ids.reshape(Q, N), d2.reshape(Q, N), live.reshape(Q, N)
        used = ids >= 0
        nq = used.sum(1)
        if k == T:
            break
        safe = np.where(used, ids, 0)
        lx = c[safe, 0] if c.shape[0] else np.zeros_like(x)
        ly = c[safe, 1] if c.shape[0] else np.zeros_like(y)
        with np.errstate(all="ignore"):
            dn = nq.astype(np.float64)
            pbx, pby = scan_sum(x, used, mutant) / dn, scan_sum(y, used, mutant) / dn
            lbx, lby = scan_sum(lx, used, mutant) / dn, scan_sum(ly, used, mutant) / dn
            if mutant == "uncentred":
                px, py, qx, qy = x, y, lx, ly
            else:
                px, py, qx, qy = x - pbx[:, None], y - pby[:, None], lx - lbx[:, None], ly - lby[:, None]
            ar = scan_sum(px * qx + py * qy, used, mutant)
            ai = scan_sum(px * qy - py * qx, used, mutant)
            h = np.sqrt(ar * ar + ai * ai)
            co, si = ar / h, ai / h
            tx = lbx - (co * pbx - si * pby)
            ty = lby - (si * pbx + co * pby)
        F = np.stack((co, si, tx, ty), axis=1)
        keep = (nq < min_nodes) | ~((h > 0) & np.isfinite(h)) | ~np.isfinite(F).all(1)
        kept |= keep & finite0
        steps += (~keep & finite0)
        X = np.where((keep | ~finite0)[:, None], X, F)
    with np.errstate(all="ignore"):
        rms = np.sqrt(scan_sum(d2, used, mutant) / nq.astype(np.float64))
    rms = np.where(nq > 0, rms, QNAN)
    node = np.where(finite0[:, None], ids, -1).astype(np.int32)
    stat = np.stack((nq, live2.sum(1), steps, np.where(finite0, kept * KEPT, NONFINITE)), axis=1).astype(np.int32)
    return {"poses": X, "node_landmark": node, "stat": stat, "rms": rms}
