"""NumPy reference of the relocalisation of scans in a landmark map (include/sgpr_landmark_relocalize.h,
sgpr_landmark_relocalize): the header's definition in float64, one rounding per operation (NumPy rounds
every ufunc on its own).  The hypotheses of a base pair are formed as one (j, j') matrix; the winner's match, the refine
stages and the rows they leave ARE landmark_align_ref.align of the one scan.  The inliers of the many hypotheses are
counted by the same gate, d2 <= r r and |mz - cz| <= tau_z, evaluated exactly on the candidates a coarse grid leaves
(cells twice the radius wide: a landmark inside the gate is never two cells away); test_landmark_relocalize_host.py
checks that count against landmark_align_ref.align with iters = 0.

relocalize(...) returns a dict with every output of the call.  relocalize(..., mutant=NAME) is the definition with one
rule altered (MUTANTS): what a subtly wrong kernel would compute; the host test proves that each one changes an output
on some case."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
from landmark_track_ref import _fma  # noqa: E402

LIMIT = aref.LIMIT
QNAN = aref.QNAN
MAX_STAGES = 16
MAX_LABELS = 64
LDS_SLOTS = 256
FOUND, KEPT, TRUNCATED, NO_HYPOTHESIS = 1, 2, 4, 8
_CHUNK = 1 << 22

# "min_base_lt", "max_base_lt", "tau_edge_lt", "tau_z_lt" (the base nodes' height test), "radius_lt" (the inlier gate),
# "sep_ge", "min_inliers_gt": the comparison of that test made strict (or, for sep, lax); "no_height": the height test
# of the two base nodes dropped; "from_node_i": the translation lays node i on landmark j instead of midpoint on midpoint;
# "ties_high": equal inliers go to the HIGHEST (i, i', j, j'); "cap_inside": a base pair is cut where the count reaches
# max_hyp; "sep_refined": the other place is measured from the refined pose; "fused_c": ux vx + uy vy with one rounding;
# "refine_unfound": the stages run on a scan that is not found; "height_i_only" / "height_ip_only": the height test of a
# hypothesis made on node i alone / on node i' alone
MUTANTS = ("min_base_lt", "max_base_lt", "tau_edge_lt", "tau_z_lt", "radius_lt", "sep_ge", "min_inliers_gt", "no_height",
           "from_node_i", "ties_high", "cap_inside", "sep_refined", "fused_c", "refine_unfound", "height_i_only",
           "height_ip_only")
STARTED_MAX = 0x7fffffff    # d_stat[q][6] saturates there


def workspace_bytes(Q, N, L, n_stages):
    """sgpr_landmark_relocalize_workspace_bytes"""
    if not 0 <= n_stages <= MAX_STAGES:
        return 0
    table = aref.workspace_bytes(Q, N, L)
    if table == 0:
        return 0

    def al(v):
        return (v + 255) & ~255
    return (n_stages + 2) * table + al(2 * MAX_LABELS * 4) + al(n_stages * MAX_LABELS * 8) + (al(Q * N * 4) if N > LDS_SLOTS else 0)


def radius_table(r, n_labels):
    r = np.atleast_1d(np.asarray(r, np.float64))
    return np.full(n_labels, r[0]) if r.size == 1 else r


def _exists(mx, my, mz, c, r, tau_z, strict=False):
    """for every point, is there a landmark of `c` [M,3] inside the gate -> bool [P]; the points are finite"""
    P = mx.size
    out = np.zeros(P, bool)
    if P == 0 or c.shape[0] == 0:
        return out
    r2 = np.float64(r) * np.float64(r)
    idx = np.arange(P)
    if np.isfinite(r) and P * c.shape[0] > (1 << 16) and np.abs(c[:, :2]).max() < 2.0 ** 28 and max(np.abs(mx).max(), np.abs(my).max()) < 2.0 ** 28:
        w = max(2.0 * float(r), 1.0)
        off, mul = np.int64(1) << 30, np.int64(1) << 31
        gx, gy = np.floor(c[:, 0] / w).astype(np.int64), np.floor(c[:, 1] / w).astype(np.int64)
        cells = np.unique(np.concatenate([(gx + dx + off) * mul + (gy + dy + off) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]))
        code = (np.floor(mx / w).astype(np.int64) + off) * mul + (np.floor(my / w).astype(np.int64) + off)
        at = np.searchsorted(cells, code)
        idx = np.flatnonzero(cells[np.minimum(at, cells.size - 1)] == code)
    step = max(1, _CHUNK // c.shape[0])
    for lo in range(0, idx.size, step):
        k = idx[lo:lo + step]
        with np.errstate(all="ignore"):
            ex = mx[k][:, None] - c[None, :, 0]
            ey = my[k][:, None] - c[None, :, 1]
            d2 = ex * ex + ey * ey
            dz = np.abs(mz[k][:, None] - c[None, :, 2])
            ok = ((d2 < r2) if strict else (d2 <= r2)) & (dz <= tau_z)
        out[k] = ok.any(1)
    return out


def count_inliers(poses, x, y, z, lab, c, elab, radius, tau_z, strict=False):
    """inliers of every hypothesis: poses f64 [H,4]; x, y, z f64 [n], lab int [n]: the LIVE nodes of the scan -> int64 [H]"""
    H = poses.shape[0]
    inl = np.zeros(H, np.int64)
    if H == 0 or x.size == 0:
        return inl
    step = max(1, _CHUNK // x.size)
    for lo in range(0, H, step):
        X = poses[lo:lo + step]
        with np.errstate(all="ignore"):
            mx = (X[:, 0:1] * x[None, :] - X[:, 1:2] * y[None, :]) + X[:, 2:3]
            my = (X[:, 1:2] * x[None, :] + X[:, 0:1] * y[None, :]) + X[:, 3:4]
            ok = np.isfinite(mx) & np.isfinite(my) & (np.abs(mx) <= LIMIT) & (np.abs(my) <= LIMIT)
        hit = np.zeros(mx.shape, bool)
        for l in np.unique(lab):
            cols = np.flatnonzero(lab == l)
            sel = ok[:, cols]
            rows, cc = np.nonzero(sel)
            if rows.size == 0:
                continue
            e = _exists(mx[:, cols][sel], my[:, cols][sel], np.broadcast_to(z[cols][None, :], sel.shape)[sel], c[elab == l],
                        radius[l], tau_z, strict)
            hit[rows, cols[cc]] = e
        inl[lo:lo + step] = hit.sum(1)
    return inl


def _one_scan(cen, lab, c, lml, lm_use, rad_in, table, P, mutant):
    """one scan -> its outputs"""
    N = lab.shape[0]
    n_labels = rad_in.size
    x, y, z = (cen[:, k].astype(np.float64) for k in range(3))
    tau_z, tau_edge = np.float64(P["tau_z"]), np.float64(P["tau_edge"])
    lab64 = lab.astype(np.int64)
    live = (lab64 >= 0) & (lab64 < n_labels)
    live[live] = rad_in[lab64[live]] > 0
    with np.errstate(all="ignore"):
        live &= np.isfinite(cen).all(1) & (np.abs(cen.astype(np.float64)) <= LIMIT).all(1)
    elab = aref.eligible(c, lml, lm_use, rad_in)
    slots = np.flatnonzero(live)

    # ---- enumeration
    hi_, hip_, hj_, hjp_, hX = [], [], [], [], []
    count = started = 0
    truncated = False
    a, b = np.triu_indices(slots.size, 1)                            # ascending (i, i')
    si, sp = slots[a], slots[b]
    with np.errstate(all="ignore"):
        ux, uy = x[sp] - x[si], y[sp] - y[si]
        lu = np.sqrt(ux * ux + uy * uy)
        adm = ((lu > P["min_base"]) if mutant == "min_base_lt" else (lu >= P["min_base"])) & \
              ((lu < P["max_base"]) if mutant == "max_base_lt" else (lu <= P["max_base"]))
    for k in np.flatnonzero(adm):
        if count >= P["max_hyp"]:
            truncated = True
            break
        started = min(started + 1, STARTED_MAX)
        i, ip = int(si[k]), int(sp[k])
        with np.errstate(all="ignore"):
            dzi, dzp = np.abs(z[i] - c[:, 2]), np.abs(z[ip] - c[:, 2])
            if mutant == "no_height":
                hi_ok = hp_ok = np.ones(c.shape[0], bool)
            elif mutant == "tau_z_lt":
                hi_ok, hp_ok = dzi < tau_z, dzp < tau_z
            else:
                hi_ok, hp_ok = dzi <= tau_z, dzp <= tau_z
            if mutant == "height_i_only":
                hp_ok = np.ones(c.shape[0], bool)
            elif mutant == "height_ip_only":
                hi_ok = np.ones(c.shape[0], bool)
        J = np.flatnonzero((elab == lab64[i]) & hi_ok)
        Jp = np.flatnonzero((elab == lab64[ip]) & hp_ok)
        if J.size == 0 or Jp.size == 0:
            continue
        step = max(1, _CHUNK // Jp.size)
        for lo in range(0, J.size, step):
            Jc = J[lo:lo + step]
            with np.errstate(all="ignore"):
                vx = c[Jp, 0][None, :] - c[Jc, 0][:, None]
                vy = c[Jp, 1][None, :] - c[Jc, 1][:, None]
                lv = np.sqrt(vx * vx + vy * vy)
                dl = np.abs(lu[k] - lv)
                ok = ((dl < tau_edge) if mutant == "tau_edge_lt" else (dl <= tau_edge)) & (Jc[:, None] != Jp[None, :])
                den = lu[k] * lv
                ok &= np.isfinite(den) & (den > 0)
            r, q = np.nonzero(ok)                                    # ascending (j, j')
            if r.size == 0:
                continue
            vx, vy, den = vx[r, q], vy[r, q], den[r, q]
            j, jp = Jc[r], Jp[q]
            with np.errstate(all="ignore"):
                if mutant == "fused_c":
                    co = np.array([_fma(ux[k], vx[t], uy[k] * vy[t]) for t in range(r.size)], np.float64) / den
                else:
                    co = (ux[k] * vx + uy[k] * vy) / den
                sn = (ux[k] * vy - uy[k] * vx) / den
                if mutant == "from_node_i":
                    pmx, pmy, lmx, lmy = x[i], y[i], c[j, 0], c[j, 1]
                else:
                    pmx, pmy = 0.5 * (x[i] + x[ip]), 0.5 * (y[i] + y[ip])
                    lmx, lmy = 0.5 * (c[j, 0] + c[jp, 0]), 0.5 * (c[j, 1] + c[jp, 1])
                tx = lmx - (co * pmx - sn * pmy)
                ty = lmy - (sn * pmx + co * pmy)
            X = np.stack((co, sn, tx, ty), axis=1)
            fin = np.isfinite(X).all(1)
            X, j, jp = X[fin], j[fin], jp[fin]
            if mutant == "cap_inside":
                room = max(P["max_hyp"] - count, 0)
                truncated |= X.shape[0] > room
                X, j, jp = X[:room], j[:room], jp[:room]
            count += X.shape[0]
            hi_.append(np.full(X.shape[0], i))
            hip_.append(np.full(X.shape[0], ip))
            hj_.append(j)
            hjp_.append(jp)
            hX.append(X)

    out = {"poses": np.full(4, QNAN), "coarse": np.full(4, QNAN), "other": np.full(4, QNAN),
           "node_landmark": np.where(live, -2, -1).astype(np.int32), "win": np.full(4, -1, np.int32), "hyp": np.int64(count),
           "rms": QNAN}
    flags = TRUNCATED if truncated else 0
    if count == 0:
        out["stat"] = np.array([0, 0, 0, live.sum(), 0, flags | NO_HYPOTHESIS, started, 0], np.int32)
        return out
    hi, hip, hj, hjp, hX = (np.concatenate(v) for v in (hi_, hip_, hj_, hjp_, hX))
    inl = count_inliers(hX, x[slots], y[slots], z[slots], lab64[slots], c, elab, rad_in, tau_z, mutant == "radius_lt")

    def first(mask):
        """the first of the masked hypotheses by the key, or -1"""
        idx = np.flatnonzero(mask)
        if idx.size == 0:
            return -1
        top = idx[inl[idx] == inl[idx].max()]
        order = np.lexsort((hjp[top], hj[top], hip[top], hi[top]))
        return int(top[order[-1] if mutant == "ties_high" else order[0]])

    w = first(np.ones(count, bool))
    found = inl[w] > P["min_inliers"] if mutant == "min_inliers_gt" else inl[w] >= P["min_inliers"]
    out["coarse"] = hX[w].copy()
    out["win"] = np.array([hi[w], hip[w], hj[w], hjp[w]], np.int32)
    stat = [int(inl[w]), 0, 0, int(live.sum()), 0, flags | (FOUND if found else 0), started, 0]
    if found or mutant == "refine_unfound":
        X = hX[w][None].copy()
        kept = refits = 0
        stages = list(table) if len(table) else [None]
        for rad in stages:
            al = aref.align(cen[None], lab[None], X, c, lml, lm_use, radius=rad_in if rad is None else rad, tau_z=tau_z,
                            iters=0 if rad is None else P["iters"], min_nodes=P["min_nodes"], n_labels=n_labels)
            X = al["poses"]
            refits += int(al["stat"][0, 2])
            kept |= int(al["stat"][0, 3]) & aref.KEPT
        out["poses"], out["node_landmark"], out["rms"] = X[0], al["node_landmark"][0], al["rms"][0]
        stat[2], stat[3], stat[4] = int(al["stat"][0, 0]), int(al["stat"][0, 1]), refits
        stat[5] |= KEPT if kept else 0
    if found:
        ref = out["poses"] if mutant == "sep_refined" else hX[w]
        with np.errstate(all="ignore"):
            dx, dy = hX[:, 2] - ref[2], hX[:, 3] - ref[3]
            d2, s2 = dx * dx + dy * dy, np.float64(P["sep"]) * np.float64(P["sep"])
            far = (d2 >= s2) if mutant == "sep_ge" else (d2 > s2)
        o = first(far)
        if o >= 0:
            stat[1] = int(inl[o])
            out["other"] = hX[o].copy()
    out["stat"] = np.array(stat, np.int32)
    return out


def relocalize(centers, labels, lm_center, lm_label, lm_use=None, radius_in=0.75, radii=(2.0, 0.75), tau_z=0.75, tau_edge=0.5,
               min_base=5.0, max_base=30.0, max_hyp=65536, min_inliers=12, sep=10.0, iters=10, min_nodes=6, n_labels=None,
               mutant=None):
    """centers f32 [Q,N,3], labels i32 [Q,N]; lm_center f64 [L,3], lm_label i32 [L], lm_use u8 [L] or None; radius_in: a
    scalar or one value per label; radii: the refine stages -> dict: poses, coarse, other f64 [Q,4], node_landmark i32
    [Q,N], stat i32 [Q,8], win i32 [Q,4], hyp i64 [Q], rms f64 [Q], num i32 [4]"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    lab = np.asarray(labels, np.int32)
    Q, N = lab.shape
    cen = np.asarray(centers, np.float32).reshape(Q, N, 3)
    rows = [np.atleast_1d(np.asarray(r, np.float64)) for r in ([] if radii is None else radii)]
    rin = np.atleast_1d(np.asarray(radius_in, np.float64))
    if n_labels is None:
        n_labels = max([r.size for r in rows + [rin] if r.size > 1], default=12)
    rad_in = radius_table(rin, n_labels)
    table = [radius_table(r, n_labels) for r in rows]
    if len(table) > MAX_STAGES:
        raise ValueError("stages")
    c = np.asarray(lm_center, np.float64).reshape(-1, 3)
    lml = np.asarray(lm_label, np.int32).reshape(-1)
    P = dict(tau_z=tau_z, tau_edge=tau_edge, min_base=np.float64(min_base), max_base=np.float64(max_base), max_hyp=int(max_hyp),
             min_inliers=int(min_inliers), sep=sep, iters=int(iters), min_nodes=int(min_nodes))
    res = [_one_scan(cen[q], lab[q], c, lml, lm_use, rad_in, table, P, mutant) for q in range(Q)]
    out = {k: np.stack([r[k] for r in res]) if Q else np.zeros((0,) + shape, dt)
           for k, shape, dt in (("poses", (4,), np.float64), ("coarse", (4,), np.float64), ("other", (4,), np.float64),
                                ("node_landmark", (N,), np.int32), ("stat", (8,), np.int32), ("win", (4,), np.int32),
                                ("hyp", (), np.int64), ("rms", (), np.float64))}
    fl = out["stat"][:, 5] if Q else np.zeros(0, np.int32)
    out["num"] = np.array([((fl & FOUND) != 0).sum(), ((fl & TRUNCATED) != 0).sum(), ((fl & NO_HYPOTHESIS) != 0).sum(), 0], np.int32)
    return out


def se2(yaw, x, y):
    return np.array([np.cos(yaw), np.sin(yaw), x, y])


def view(lm, pose, noise=None):
    """the landmarks lm [M,3] as a scan at `pose` (sensor into map) sees them -> float32 [M,3]"""
    c, s, tx, ty = pose
    dx, dy = lm[:, 0] - tx, lm[:, 1] - ty
    out = np.stack((c * dx + s * dy, c * dy - s * dx, lm[:, 2]), axis=1)
    if noise is not None:
        out[:, :2] += noise
    return out.astype(np.float32)


def aliased_map(gap=200.0, seed=5, n=14, labels=3):
    """the same constellation of n landmarks planted twice, `gap` metres apart; the second copy lacks its last landmark.
    -> dict: lm f64 [2 n - 1, 3], lm_label, a scan of the constellation (centers f32 [1,n,3], labels i32 [1,n]) and its
    true pose in the first copy"""
    rng = np.random.default_rng(seed)
    base = np.concatenate((rng.uniform(-20.0, 20.0, size=(n, 2)), rng.uniform(-0.3, 0.3, size=(n, 1))), axis=1)
    lab = (np.arange(n) % labels).astype(np.int32)
    second = base[:-1] + np.array([gap, 0.0, 0.0])
    truth = se2(0.4, 1.5, -2.0)
    cen = view(base, truth, rng.normal(0, 0.01, size=(n, 2)))
    return {"lm": np.concatenate((base, second)), "lm_label": np.concatenate((lab, lab[:-1])), "centers": cen[None],
            "labels": lab[None], "truth": truth, "n": n, "gap": gap}


# ------------------------------------------------------------------ hand-made cases (the host and the GPU tests share them)
def _scan(points, labels, N=None):
    """points [n,3], labels [n] padded to N slots (centre 0, label -1) -> (f32 [1,N,3], i32 [1,N])"""
    pts, lab = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(labels, np.int32).reshape(-1)
    N = pts.shape[0] if N is None else N
    cen, out = np.zeros((1, N, 3), np.float32), np.full((1, N), -1, np.int32)
    cen[0, :pts.shape[0]], out[0, :lab.size] = pts, lab
    return cen, out


def exact_world():
    """Binary-exact coordinates; the scan is the map seen from the identity.  Landmarks (all label 0): A B C D with
    |AB| = |CD| = 10 exactly, A and B 0.75 above / below their nodes; G, whose node lies 0.75 beside it; E F 10.5 apart;
    A2 B2 = A B moved by (64, 0).  min_base = max_base = 10: the base pairs are (A', B') and (C', D')."""
    lm = np.array([[0, 0, 0.75], [6, 8, -0.75], [6, 0, 0], [0, 8, 0], [20, 0, 0], [100, 0, 0], [110.5, 0, 0], [64, 0, 0.75],
                   [70, 8, -0.75]], np.float64)
    cen, lab = _scan([[0, 0, 0], [6, 8, 0], [6, 0, 0], [0, 8, 0], [20, 0.75, 0]], [0] * 5, N=8)
    kw = dict(radius_in=0.75, radii=(), tau_z=0.75, tau_edge=0.5, min_base=10.0, max_base=10.0, min_inliers=5, sep=64.0,
              min_nodes=2, n_labels=2)
    return {"centers": cen, "labels": lab, "lm": lm, "lm_label": np.zeros(9, np.int32), "kw": kw}


def line_world(n, extra=3):
    """n landmarks of label 0 at (100 k, 0) and n of label 1 at (100 k + 10, 0): the base pair (node of label 0, node of
    label 1, 10 apart) has exactly n hypotheses, one per j, all with the same inliers - the lowest (j, j') wins"""
    k = np.arange(n, dtype=np.float64)
    lm = np.zeros((2 * n, 3))
    lm[0::2, 0], lm[1::2, 0] = 100.0 * k, 100.0 * k + 10.0
    lml = np.tile(np.array([0, 1], np.int32), n)
    cen, lab = _scan([[0, 0, 0], [10, 0, 0]] + [[0.25 * (t + 1), 40.0, 0] for t in range(extra)], [0, 1] + [2] * extra, N=8)
    kw = dict(radius_in=0.75, radii=(), min_base=5.0, max_base=30.0, min_inliers=2, sep=50.0, min_nodes=2, n_labels=3)
    return {"centers": cen, "labels": lab, "lm": lm, "lm_label": lml, "kw": kw}


def lattice_world(side=6, pitch=8.0, N=8):
    """side x side landmarks of one label on a square lattice, a scan of a 2 x 2 block of it: every translate and quarter
    turn of the block fits as well as the truth - equal inliers, the key order decides"""
    g = np.arange(side, dtype=np.float64) * pitch
    lm = np.stack((np.repeat(g, side), np.tile(g, side), np.zeros(side * side)), axis=1)
    cen, lab = _scan([[0, 0, 0], [pitch, 0, 0], [0, pitch, 0], [pitch, pitch, 0]], [0] * 4, N=N)
    kw = dict(radius_in=0.75, radii=(), min_base=5.0, max_base=12.0, min_inliers=4, sep=10.0, min_nodes=2, n_labels=1)
    return {"centers": cen, "labels": lab, "lm": lm, "lm_label": np.zeros(side * side, np.int32), "kw": kw}


def dense_world(side=20, pitch=2.0):
    """side x side landmarks of one label, 2 m apart, and a scan of six of them: a base pair has hundreds of hypotheses,
    several j' per j and more j than one chunk of lanes"""
    g = np.arange(side, dtype=np.float64) * pitch
    lm = np.stack((np.repeat(g, side), np.tile(g, side), np.zeros(side * side)), axis=1)
    pick = [0, 3, 45, 64, 130, 207]
    truth = se2(0.3, 1.0, -2.0)
    cen, lab = _scan(view(lm[pick], truth), [0] * 6, N=70)
    kw = dict(radius_in=0.5, radii=(1.0, 0.5), min_base=4.0, max_base=10.0, tau_edge=0.25, min_inliers=5, sep=3.0, min_nodes=2,
              n_labels=1)
    return {"centers": cen, "labels": lab, "lm": lm, "lm_label": np.zeros(side * side, np.int32), "kw": kw, "truth": truth}


def run(w, **over):
    """relocalize on a world dict, its kw overridden"""
    kw = dict(w["kw"])
    lm_use = over.pop("lm_use", w.get("lm_use"))
    kw.update(over)
    return relocalize(w["centers"], w["labels"], w["lm"], w["lm_label"], lm_use, **kw)


def up(v):
    return np.nextafter(np.float64(v), np.inf)


def down(v):
    return np.nextafter(np.float64(v), -np.inf)


def hand_cases():
    """name -> (world, overrides): every hand-made case the tests run, on the reference and on the GPU"""
    ex, la, al = exact_world(), lattice_world(), aliased_map()
    alw = {"centers": al["centers"], "labels": al["labels"], "lm": al["lm"], "lm_label": al["lm_label"],
           "kw": dict(radii=(2.0, 0.75), min_inliers=8, n_labels=3)}
    masked = np.ones(al["lm"].shape[0], np.uint8)
    masked[al["n"]:] = 0
    cases = {"exact": (ex, {}),
             "min_base_past": (ex, dict(min_base=up(10.0), max_base=12.0)), "min_base_at_wide": (ex, dict(max_base=12.0)),
             "max_base_past": (ex, dict(min_base=9.0, max_base=down(10.0))), "max_base_at_wide": (ex, dict(min_base=9.0)),
             "tau_edge_past": (ex, dict(tau_edge=down(0.5))), "tau_z_past": (ex, dict(tau_z=down(0.75))),
             "radius_past": (ex, dict(radius_in=down(0.75))), "sep_past": (ex, dict(sep=down(64.0))),
             "sep_zero": (ex, dict(sep=0.0)), "sep_inf": (ex, dict(sep=np.inf)),
             "min_inliers_past": (ex, dict(min_inliers=6)), "staged": (ex, dict(radii=(2.0, 0.75), iters=3)),
             "lattice": (la, {}), "lattice_stages": (la, dict(radii=(1.0,), iters=2)),
             "aliased": (alw, {}), "aliased_masked": (alw, dict(lm_use=masked))}
    # the height test is made on BOTH base nodes: only landmark A (under node i), or only B (under node i'), one double out
    for name, row, z in (("tau_z_j_only", 0, up(0.75)), ("tau_z_jp_only", 1, down(-0.75))):
        w = dict(ex)
        w["lm"] = ex["lm"].copy()
        w["lm"][row, 2] = z
        cases[name] = (w, dict(min_inliers=3))
    # den > 0: two coincident landmarks under two nodes a quarter metre apart, min_base = 0; and two coincident nodes
    co = dict(ex)
    co["lm"] = np.concatenate((ex["lm"], [[50.0, 50.0, 0.0], [50.0, 50.0, 0.0]]))
    co["lm_label"] = np.zeros(11, np.int32)
    co["centers"], co["labels"] = _scan([[0, 0, 0], [0.25, 0, 0], [0.25, 0, 0], [6, 8, 0]], [0] * 4, N=8)
    cases["coincident"] = (co, dict(min_base=0.0, max_base=10.0, min_inliers=2))
    # L = 0, 1, 2
    for L in (0, 1, 2):
        w = dict(ex)
        w["lm"], w["lm_label"] = ex["lm"][:L], ex["lm_label"][:L]
        cases["L%d" % L] = (w, dict(min_inliers=2))
    # fewer than two live nodes; a label of radius 0; NaNs
    one = dict(ex)
    one["labels"] = ex["labels"].copy()
    one["labels"][0, 1:] = -1
    cases["one_live_node"] = (one, {})
    two = dict(ex)
    two["labels"] = ex["labels"].copy()
    two["labels"][0, 2:5] = 1
    two["lm_label"] = np.array([0, 0, 1, 1, 1, 0, 0, 0, 0], np.int32)
    cases["two_labels"] = (two, dict(min_inliers=2))
    cases["radius_zero"] = (two, dict(min_inliers=2, radius_in=np.array([0.75, 0.0])))
    cases["stage_radius_zero"] = (two, dict(min_inliers=2, radii=(np.array([2.0, 0.0]), np.array([0.75, 0.75])), iters=2))
    for name, where in (("nan_node", "node"), ("nan_landmark", "lm"), ("nan_padding", "pad")):
        w = dict(ex)
        w["centers"], w["lm"] = ex["centers"].copy(), ex["lm"].copy()
        if where == "node":
            w["centers"][0, 2, 0] = np.nan
        elif where == "lm":
            w["lm"][2, 1] = np.nan
        else:
            w["centers"][0, 6] = np.nan
        cases[name] = (w, dict(min_inliers=3))
    return cases


def mutant_cases():
    """name -> (world, overrides): the cases on which the host test shows that every mutant of MUTANTS changes an output;
    the GPU test sends each of them through the kernel"""
    ex, la, al = exact_world(), lattice_world(), hand_cases()["aliased"][0]
    high = dict(ex)
    high["lm"] = ex["lm"].copy()
    high["lm"][7:, 2] += 2.0                                     # A2, B2 out of the base nodes' height
    tilt = dict(ex)                                              # the map seen from a pose that is not the identity
    tilt["centers"] = ex["centers"].copy()
    tilt["centers"][0, :5, :2] = view(ex["lm"][:5], se2(0.3, 0.1, 0.2))[:, :2]
    cases = {"exact": (ex, {}), "lattice": (la, {}), "lattice_sep": (la, dict(sep=8.0)), "lattice_cap": (la, dict(max_hyp=100)),
             "high": (high, {}), "tilt": (tilt, dict(min_base=9.5, max_base=10.5, radii=(2.0, 0.75), min_inliers=4)),
             "unfound": (ex, dict(min_inliers=6, radii=(2.0,))), "aliased": (al, dict(sep=199.0)),
             "height_j": hand_cases()["tau_z_j_only"], "height_jp": hand_cases()["tau_z_jp_only"]}
    # eight scans of the aliased constellation at eight yaws: some winner's c rounds differently when fused
    turned = dict(al)
    turned["centers"] = np.stack([view(al["lm"][:14], se2(0.05 + 0.37 * k, 1.0 * k, -2.0 * k)) for k in range(8)])
    turned["labels"] = np.repeat(al["labels"], 8, 0)
    cases["turned"] = (turned, {})
    # two nodes of the lattice block half a metre off: the coarse pose of (0, 1) is the identity, the refit moves it a
    # decimetre - the translates exactly 8 m from the coarse pose are more than 8 m from the refined one
    shifted = dict(la)
    shifted["centers"] = la["centers"].copy()
    shifted["centers"][0, 2:4, 0] += 0.5
    cases["shifted"] = (shifted, dict(sep=8.0, radii=(0.75,), iters=2))
    return cases
