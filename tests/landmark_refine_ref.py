"""NumPy reference of the landmark refinement (include/sgpr_landmark_refine.h, sgpr_landmark_refine): the
header's definition in float64, one rounding per operation (NumPy rounds every ufunc on its own), the sums over a
landmark and over the map in int64 / uint64, the scan sums W as 64 partials and the halving tree, exactly as defined.

refine(...) returns a dict with every output of the call.  refine(..., mutant=NAME) is the definition with one rule
altered (MUTANTS): what a subtly wrong kernel would compute; tests/test_landmark_refine_host.py proves that each one
changes an output on some case."""
import fractions

import numpy as np

FIX = 16777216.0            # 2^24
LIMIT = 137438953472.0      # 2^37
D2_CAP = 1048576.0          # 2^20
LANES = 64
SCALARS = 32

# "sequential": the scan sums in slot order instead of W; "fused_ar": p'x l'x + p'y l'y with the first product fused into
# the sum; "uncentred": the moments of p, l instead of p', l'; "gauss_seidel": a scan's new pose moves the centres before
# the next scan is fitted; "float_centres": centres by a sequential float64 sum in node order
MUTANTS = ("sequential", "fused_ar", "uncentred", "gauss_seidel", "float_centres")


def workspace_bytes(G, N, L):
    """sgpr_landmark_refine_workspace_bytes"""
    if G < 0 or N < 0 or L < 0 or G * N == 0 or G * N > 0x7fffffff:
        return 0

    def al(v):
        return (v + 255) & ~255
    return al(2 * 3 * L * 8) + al(SCALARS * 8) + 2 * al(G * 32)


def scan_sum(v, used, mutant=None):
    """W(v) of every scan: v, used [G,N] -> float64 [G]"""
    v = np.where(used, v, 0.0)        # (a partial starts at +0.0 and so is never -0.0: adding +0.0 is skipping the slot)
    G, N = v.shape
    if mutant == "sequential":
        out = np.zeros(G)
        for n in range(N):
            out = out + v[:, n]
        return out
    rounds = (N + LANES - 1) // LANES
    pad = np.zeros((G, rounds * LANES))
    pad[:, :N] = v
    pad = pad.reshape(G, rounds, LANES)
    part = np.zeros((G, LANES))
    for r in range(rounds):
        part = part + pad[:, r]
    h = LANES // 2
    while h >= 1:
        part = part[:, :h] + part[:, h:2 * h]
        h //= 2
    return part[:, 0]


def _fma(a, b, c):
    """a b + c rounded once, elementwise (exact rational arithmetic; the mutation test only, on finite values)"""
    out = np.empty(a.shape)
    for i in np.ndindex(a.shape):
        out[i] = float(fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i])))
    return out


def centres(x, y, ids, ok, L, X, mutant=None):
    """the used nodes under poses X and the centres of their landmarks -> (used [G,N], mx, my [G,N], cnt int64 [L],
    cx, cy float64 [L])"""
    c, s, tx, ty = (X[:, k][:, None] for k in range(4))
    with np.errstate(all="ignore"):
        mx = (c * x - s * y) + tx
        my = (s * x + c * y) + ty
        used = ok & np.isfinite(X).all(1)[:, None] & np.isfinite(mx) & np.isfinite(my) & (np.abs(mx) <= LIMIT) & (np.abs(my) <= LIMIT)
        idu = ids[used]
        cnt = np.bincount(idu, minlength=L).astype(np.int64)
        Sx, Sy = np.zeros(L, np.int64), np.zeros(L, np.int64)
        np.add.at(Sx, idu, np.rint(mx[used] * FIX).astype(np.int64))
        np.add.at(Sy, idu, np.rint(my[used] * FIX).astype(np.int64))
        den = cnt.astype(np.float64) * FIX
        cx, cy = Sx.astype(np.float64) / den, Sy.astype(np.float64) / den
        if mutant == "float_centres":
            cx, cy = np.zeros(L), np.zeros(L)
            for i, vx, vy in zip(idu, mx[used], my[used]):
                cx[i] = cx[i] + vx
                cy[i] = cy[i] + vy
            cx, cy = cx / cnt.astype(np.float64), cy / cnt.astype(np.float64)
    return used, mx, my, cnt, cx, cy


def fit(x, y, used, lx, ly, X, fixed, min_nodes, mutant=None):
    """the fit of every scan against the centres lx, ly [G,N] of its nodes -> (X_next [G,4], kept bool [G])"""
    ng = used.sum(1)
    with np.errstate(all="ignore"):
        dn = ng.astype(np.float64)
        pbx, pby = scan_sum(x, used, mutant) / dn, scan_sum(y, used, mutant) / dn
        lbx, lby = scan_sum(lx, used, mutant) / dn, scan_sum(ly, used, mutant) / dn
        if mutant == "uncentred":
            px, py, qx, qy = x, y, lx, ly
        else:
            px, py, qx, qy = x - pbx[:, None], y - pby[:, None], lx - lbx[:, None], ly - lby[:, None]
        if mutant == "fused_ar":
            safe = [np.where(used, v, 0.0) for v in (px, py, qx, qy)]
            t_ar = _fma(safe[0], safe[2], safe[1] * safe[3])
        else:
            t_ar = px * qx + py * qy
        t_ai = px * qy - py * qx
        ar, ai = scan_sum(t_ar, used, mutant), scan_sum(t_ai, used, mutant)
        h = np.sqrt(ar * ar + ai * ai)
        c, s = ar / h, ai / h
        tx = lbx - (c * pbx - s * pby)
        ty = lby - (s * pbx + c * pby)
    F = np.stack((c, s, tx, ty), axis=1)
    keep = fixed | (ng < min_nodes) | ~((h > 0) & np.isfinite(h)) | ~np.isfinite(F).all(1)
    return np.where(keep[:, None], X, F), keep


def refine(centers, node_landmark, poses, lm_use, fixed=None, iters=10, min_nodes=6, mutant=None):
    """centers f32 [G,N,3], node_landmark i32 [G,N], poses f64 [G,4], lm_use u8 [L] -> dict: poses f64 [G,4],
    cost f64 [iters+1], info i32 [4]"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    ids = np.asarray(node_landmark, np.int64)
    G, N = ids.shape
    use = np.asarray(lm_use, np.uint8).reshape(-1)
    L = use.size
    cen = np.asarray(centers, np.float32).reshape(G, N, 3).astype(np.float64)
    x, y = cen[..., 0], cen[..., 1]
    X = np.array(np.asarray(poses, np.float64).reshape(G, 4))
    fixed = np.zeros(G, bool) if fixed is None else np.asarray(fixed).reshape(G) != 0
    ok = (ids >= 0) & (ids < L)
    ids = np.where(ok, ids, 0)
    if L:
        ok &= use[ids] != 0
    T = int(iters)
    cost = np.zeros(T + 1)
    info = np.zeros(4, np.int32)
    for k in range(T + 1):
        used, mx, my, cnt, cx, cy = centres(x, y, ids, ok, L, X, mutant)
        with np.errstate(all="ignore"):
            lx, ly = cx[ids] if L else np.zeros_like(x), cy[ids] if L else np.zeros_like(y)
            ex, ey = mx[used] - lx[used], my[used] - ly[used]
            d2 = ex * ex + ey * ey
            Q = np.sum(np.rint(np.minimum(d2, D2_CAP) * FIX).astype(np.uint64), dtype=np.uint64)
            n = int(used.sum())
            cost[k] = np.sqrt(np.float64(Q) / (np.float64(n) * FIX)) if n else np.nan
        if k == T:
            info[0], info[1] = n, int((cnt > 0).sum())
            break
        if mutant == "gauss_seidel":
            nxt, keep = X.copy(), np.zeros(G, bool)
            for g in range(G):
                used, mx, my, cnt, cx, cy = centres(x, y, ids, ok, L, nxt, mutant)
                one, kept = fit(x[g:g + 1], y[g:g + 1], used[g:g + 1], cx[ids[g:g + 1]], cy[ids[g:g + 1]], nxt[g:g + 1],
                                fixed[g:g + 1], min_nodes)
                nxt[g], keep[g] = one[0], kept[0]
        else:
            nxt, keep = fit(x, y, used, lx, ly, X, fixed, min_nodes, mutant)
        if k == T - 1:
            info[2], info[3] = int((~keep).sum()), int((keep & ~fixed).sum())
        X = nxt
    return {"poses": X, "cost": cost, "info": info}
