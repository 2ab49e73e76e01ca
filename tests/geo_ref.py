"""NumPy reference of the geometric verification of loop-closure candidates (include/sgpr.h, sgpr_verify_pairs;
DESIGN.md §19): the definition in float32 / float64, one rounding per operation, explicit sequential loops wherever the
order of a sum matters.  Hypotheses are evaluated vectorised (a maximum over one key does not depend on the order);
NumPy rounds every float32 ufunc on its own, there is no fused multiply-add anywhere.

verify_pair(...) returns one record of dtype RESULT; verify_pairs(...) the records of a pair list, index checks
included.  verify_pair(..., mutant=NAME) is the definition with one rule altered (MUTANTS): what a subtly wrong kernel
would compute, used by tests/test_verify_boundary_host.py to prove that the cases of tests/verify_cases.py sit on the
rules."""
import numpy as np

RESULT = np.dtype([("inliers", "<i4"), ("inliers_refined", "<i4"), ("base", "<i4", (4,)), ("hypotheses", "<u4"),
                   ("flags", "<u4"), ("coarse", "<f4", (4,)), ("refined", "<f8", (4,)), ("rmse", "<f8")])
INVALID_INDEX, NO_HYPOTHESIS, TRUNCATED, NONFINITE = 1, 2, 4, 8
DEFAULTS = dict(tau_edge=0.5, tau_in=0.6, tau_z=1.0, min_base=5.0, max_hyp=65536)
_EVAL_CHUNK = 1 << 21   # hypotheses x correspondences evaluated per NumPy pass

f32 = np.float32

# verify_pair(..., mutant=NAME): the definition with exactly ONE rule altered - what a subtly wrong kernel would compute.
# tests/test_verify_boundary_host.py proves with them that every case of tests/verify_cases.py sits on its rule.
MUTANTS = ("min_base_strict", "edge_strict", "inlier_strict", "z_strict", "inlier_fused", "base_len_fused",
           "flush_subnormals", "best_tie_highest", "match_tie_last", "cap_after", "cap_strict", "lv_zero_ok")
_TINY = f32(1.1754943508222875e-38)     # the smallest normal float32


def _ftz(x):
    """Flush subnormal float32 values to zero (mutant flush_subnormals)."""
    x = np.asarray(x, f32)
    return np.where(np.abs(x) < _TINY, f32(0), x).astype(f32)


def _sumsq(x, y, mutant, which):
    """x x + y y in float32.  The definition rounds both products and the sum; mutant `which` fuses the first product
    into the sum (one rounding of x x + round(y y): exact in float64 up to a double rounding nobody relies on), and
    flush_subnormals flushes the inlier distance's products and sum."""
    if mutant == which:
        x64, yy = np.asarray(x, np.float64), np.asarray(y * y, np.float64)
        return (x64 * x64 + yy).astype(f32)
    if mutant == "flush_subnormals" and which == "inlier_fused":
        return _ftz(_ftz(x * x) + _ftz(y * y))
    return x * x + y * y


def _within(d2, tin2, dz, tau_z, mutant):
    """The inlier rule: d2 <= tin2 and |dz| <= tau_z."""
    if mutant == "flush_subnormals":
        tin2 = _ftz(tin2)
    a = d2 < tin2 if mutant == "inlier_strict" else d2 <= tin2
    b = dz < tau_z if mutant == "z_strict" else dz <= tau_z
    return a & b


def _empty(flags, hypotheses=0):
    r = np.zeros((), dtype=RESULT)
    r["base"] = -1
    r["coarse"] = np.nan
    r["refined"] = np.nan
    r["rmse"] = np.nan
    r["flags"] = flags
    r["hypotheses"] = hypotheses
    return r


def _transform(ax, ay, bx, by, i, i2, j, j2, mutant=None):
    """The coarse transform of hypotheses (arrays of slot indices): float32, every operation rounded on its own."""
    ux, uy = ax[i2] - ax[i], ay[i2] - ay[i]
    vx, vy = bx[j2] - bx[j], by[j2] - by[j]
    lu = np.sqrt(_sumsq(ux, uy, mutant, "base_len_fused"))
    lv = np.sqrt(_sumsq(vx, vy, mutant, "base_len_fused"))
    den = lu * lv
    c = (ux * vx + uy * vy) / den
    s = (ux * vy - uy * vx) / den
    max_, may = f32(0.5) * (ax[i] + ax[i2]), f32(0.5) * (ay[i] + ay[i2])
    mbx, mby = f32(0.5) * (bx[j] + bx[j2]), f32(0.5) * (by[j] + by[j2])
    tx = mbx - (c * max_ - s * may)
    ty = mby - (s * max_ + c * may)
    return c, s, tx, ty


def _matches(ax, ay, az, la, bx, by, bz, lb, ra, rb, c, s, tx, ty, tin2, tau_z, mutant=None):
    """For one float32 transform: per real node p of A (ascending) the matched q(p) or -1 - the qualifying q with the
    smallest dx*dx + dy*dy, ties to the lowest q (rb ascends and argmin takes the first minimum)."""
    out = []
    for p in ra:
        px = (c * ax[p] - s * ay[p]) + tx
        py = (s * ax[p] + c * ay[p]) + ty
        qs = rb[lb[rb] == la[p]]
        dx, dy = px - bx[qs], py - by[qs]
        d2 = _sumsq(dx, dy, mutant, "inlier_fused")
        ok = _within(d2, tin2, np.abs(az[p] - bz[qs]), tau_z, mutant)
        if not ok.any():
            out.append(-1)
        elif mutant == "match_tie_last":
            out.append(int(qs[ok][len(d2[ok]) - 1 - np.argmin(d2[ok][::-1])]))
        else:
            out.append(int(qs[ok][np.argmin(d2[ok])]))
    return out


def verify_pair(ca, la, cb, lb, tau_edge=0.5, tau_in=0.6, tau_z=1.0, min_base=5.0, max_hyp=65536, mutant=None):
    """One pair: ca / cb [N, 3] float32 centres, la / lb [N] int32 labels (< 0: padding) -> a RESULT record.
    mutant: None (the definition) or one name of MUTANTS (the definition with that one rule altered)."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    with np.errstate(all="ignore"):
        return _verify_pair(np.asarray(ca, f32), np.asarray(la, np.int32), np.asarray(cb, f32), np.asarray(lb, np.int32),
                            f32(tau_edge), f32(tau_in), f32(tau_z), f32(min_base), int(max_hyp), mutant)


def _verify_pair(ca, la, cb, lb, tau_edge, tau_in, tau_z, min_base, max_hyp, mutant=None):
    ra, rb = np.flatnonzero(la >= 0), np.flatnonzero(lb >= 0)
    if not (np.isfinite(ca[ra]).all() and np.isfinite(cb[rb]).all()):
        return _empty(NONFINITE)
    ax, ay, az = ca[:, 0].copy(), ca[:, 1].copy(), ca[:, 2].copy()
    bx, by, bz = cb[:, 0].copy(), cb[:, 1].copy(), cb[:, 2].copy()
    tin2 = tau_in * tau_in
    # B's real slots grouped by label (slots ascending inside a label); every A node's range of it
    order = rb[np.argsort(lb[rb], kind="stable")]
    slab = lb[order]
    start = {int(p): int(np.searchsorted(slab, la[p], "left")) for p in ra}
    end = {int(p): int(np.searchsorted(slab, la[p], "right")) for p in ra}
    # the same-label correspondences (p, q), grouped by p; nodes of A without one can never be inliers
    cp = np.concatenate([np.full(end[int(p)] - start[int(p)], p) for p in ra] + [np.zeros(0, np.int64)]).astype(np.int64)
    cq = np.concatenate([order[start[int(p)]:end[int(p)]] for p in ra] + [np.zeros(0, np.int64)]).astype(np.int64)
    zabs = np.abs(az[cp] - bz[cq])
    groups = np.flatnonzero(np.r_[True, cp[1:] != cp[:-1]]) if cp.size else np.zeros(0, np.int64)

    count, truncated = 0, False
    best_key, best = None, None
    for n_i, i in enumerate(ra):
        if truncated:
            break
        i = int(i)
        if mutant != "cap_after" and (count > max_hyp if mutant == "cap_strict" else count >= max_hyp):
            truncated = n_i < len(ra) - 1          # (a base pair would still have been started)
            break
        i2s = ra[n_i + 1:]
        if i2s.size == 0:
            break
        js = order[start[i]:end[i]]
        n2 = np.array([end[int(p)] - start[int(p)] for p in i2s], np.int64)
        # candidate grid: every (i', j') with j' in the range of la[i'], crossed with j in the range of la[i]
        i2r = np.repeat(i2s, n2)
        off = np.arange(int(n2.sum())) - np.repeat(np.cumsum(n2) - n2, n2)
        j2r = order[np.repeat(np.array([start[int(p)] for p in i2s], np.int64), n2) + off] if off.size else off
        ux, uy = ax[i2s] - ax[i], ay[i2s] - ay[i]
        lu_b = np.sqrt(_sumsq(ux, uy, mutant, "base_len_fused"))            # per base pair
        H_i2 = np.tile(i2r, js.size)
        H_j2 = np.tile(j2r, js.size)
        H_j = np.repeat(js, i2r.size)
        lu = np.tile(np.repeat(lu_b, n2), js.size)
        vx, vy = bx[H_j2] - bx[H_j], by[H_j2] - by[H_j]
        lv = np.sqrt(_sumsq(vx, vy, mutant, "base_len_fused"))
        # (den = lu lv > 0: neither length is zero and their product does not underflow - c and s are never 0 / 0)
        adm = (H_j != H_j2) & (lu > min_base if mutant == "min_base_strict" else lu >= min_base)
        if mutant != "lv_zero_ok":
            adm &= lu * lv > 0
        adm &= np.abs(lu - lv) < tau_edge if mutant == "edge_strict" else np.abs(lu - lv) <= tau_edge
        # the cap: base pairs in ascending order, stop before the first one that starts with >= max_hyp evaluated
        per_base = np.bincount(np.searchsorted(i2s, H_i2[adm]), minlength=i2s.size)
        before = count + np.cumsum(per_base) - per_base
        if mutant == "cap_after":                  # tested after a base pair: that pair is still evaluated
            stop = np.flatnonzero(before + per_base >= max_hyp)
        else:
            stop = np.flatnonzero(before > max_hyp if mutant == "cap_strict" else before >= max_hyp)
        if stop.size:
            truncated = True
            n_keep = stop[0] + 1 if mutant == "cap_after" else stop[0]
            keep_i2 = i2s[:n_keep]
            adm &= np.isin(H_i2, keep_i2)
            count = int(before[stop[0]] + (per_base[stop[0]] if mutant == "cap_after" else 0))
        else:
            count += int(per_base.sum())
        hi2, hj, hj2 = H_i2[adm], H_j[adm], H_j2[adm]
        if hi2.size == 0:
            continue
        hi = np.full(hi2.size, i, np.int64)
        c, s, tx, ty = _transform(ax, ay, bx, by, hi, hi2, hj, hj2, mutant)
        inl = np.zeros(hi2.size, np.int64)
        if cp.size:
            step = max(1, _EVAL_CHUNK // cp.size)
            for h0 in range(0, hi2.size, step):
                sl = slice(h0, h0 + step)
                cc, ss, ttx, tty = c[sl, None], s[sl, None], tx[sl, None], ty[sl, None]
                px = (cc * ax[cp] - ss * ay[cp]) + ttx
                py = (ss * ax[cp] + cc * ay[cp]) + tty
                dx, dy = px - bx[cq], py - by[cq]
                ok = _within(_sumsq(dx, dy, mutant, "inlier_fused"), tin2, zabs, tau_z, mutant)
                inl[sl] = np.logical_or.reduceat(ok, groups, axis=1).sum(1)
        packed = (hi << 24) | (hi2 << 16) | (hj << 8) | hj2
        key = (inl << 32) | (packed if mutant == "best_tie_highest" else 0xffffffff - packed)
        w = int(np.argmax(key))
        if best_key is None or int(key[w]) > best_key:
            best_key = int(key[w])
            best = (i, int(hi2[w]), int(hj[w]), int(hj2[w]), int(inl[w]))
    if best is None:
        return _empty(NO_HYPOTHESIS)

    r = np.zeros((), dtype=RESULT)
    i, i2, j, j2, inl = best
    r["inliers"] = inl
    r["base"] = (i, i2, j, j2)
    r["hypotheses"] = count
    r["flags"] = TRUNCATED if truncated else 0
    idx = [np.array([v]) for v in (i, i2, j, j2)]
    c, s, tx, ty = (v[0] for v in _transform(ax, ay, bx, by, *idx, mutant))
    r["coarse"] = (c, s, tx, ty)
    m = _matches(ax, ay, az, la, bx, by, bz, lb, ra, rb, c, s, tx, ty, tin2, tau_z, mutant)
    pq = [(int(p), int(q)) for p, q in zip(ra, m) if q >= 0]
    assert len(pq) == inl, (len(pq), inl)
    # one least-squares step in float64 (Python floats: every operation rounded on its own), sums in ascending p
    n = len(pq)
    A = [(float(ax[p]), float(ay[p])) for p, _ in pq]
    B = [(float(bx[q]), float(by[q])) for _, q in pq]
    rc, rs, rtx, rty = float(c), float(s), float(tx), float(ty)
    if n >= 2:
        sax = say = sbx = sby = 0.0
        for (x, y), (u, v) in zip(A, B):
            sax = sax + x
            say = say + y
            sbx = sbx + u
            sby = sby + v
        cax, cay, cbx, cby = sax / n, say / n, sbx / n, sby / n
        D = X = 0.0
        for (x, y), (u, v) in zip(A, B):
            xa, ya, xb, yb = x - cax, y - cay, u - cbx, v - cby
            D = D + (xa * xb + ya * yb)
            X = X + (xa * yb - ya * xb)
        nrm = float(np.sqrt(np.float64(D * D + X * X)))
        if nrm != 0.0:
            rc, rs = D / nrm, X / nrm
            rtx = cbx - (rc * cax - rs * cay)
            rty = cby - (rs * cax + rc * cay)
    r["refined"] = (rc, rs, rtx, rty)
    if n == 0:
        r["rmse"] = np.nan
    else:
        ssq = 0.0
        for (x, y), (u, v) in zip(A, B):
            dx = ((rc * x - rs * y) + rtx) - u
            dy = ((rs * x + rc * y) + rty) - v
            ssq = ssq + (dx * dx + dy * dy)
        r["rmse"] = float(np.sqrt(np.float64(ssq / n)))
    m2 = _matches(ax, ay, az, la, bx, by, bz, lb, ra, rb, f32(rc), f32(rs), f32(rtx), f32(rty), tin2, tau_z,
                  mutant)
    r["inliers_refined"] = sum(1 for q in m2 if q >= 0)
    return r


def verify_pairs(centers_a, labels_a, centers_b, labels_b, idx_a, idx_b, **tol):
    """The records of a pair list: centers [G, N, 3], labels [G, N]; an index outside its graph set gives a zeroed record
    with INVALID_INDEX."""
    out = np.zeros(len(idx_a), dtype=RESULT)
    for n, (a, b) in enumerate(zip(idx_a, idx_b)):
        if not (0 <= a < len(centers_a) and 0 <= b < len(centers_b)):
            out[n]["flags"] = INVALID_INDEX
            continue
        out[n] = verify_pair(centers_a[a], labels_a[a], centers_b[b], labels_b[b], **tol)
    return out


def equal_records(x, y):
    """Field-by-field bit equality of two RESULT arrays, NaN payloads comparing as NaN.  Returns the differing fields."""
    bad = []
    for name in RESULT.names:
        a, b = np.asarray(x[name]), np.asarray(y[name])
        if a.dtype.kind == "f":
            w = "<u4" if a.dtype.itemsize == 4 else "<u8"
            same = (a.view(w) == b.view(w)) | (np.isnan(a) & np.isnan(b))
        else:
            same = a == b
        if not np.all(same):
            bad.append(name)
    return bad
