"""sgpr_posegraph_optimize (include/sgpr_posegraph.h) in NumPy, operation by operation: the two-stage
linear planar pose-graph solve the HIP kernel must reproduce bit for bit.

All arithmetic is float64 and every operation is rounded on its own (NumPy never fuses a multiply with an add).  A
complex number is a pair of float64 arrays; the products are written out so that their order of operations is the
header's.  The keyword switches after `rel_tol` exist for the mutation tests only: each turns one rule of the definition
into a plausible other one.
"""
import fractions

import numpy as np

SEGMENT = 64
CHUNK = 1024
MAX_SCANS, MAX_CLOSURES, MAX_ITERS, SESSION_MAX = 65536, 16384, 65536, 64
NONFINITE, NO_ANCHOR, DEGENERATE = 1, 2, 4
CONVERGED, STOP_MAX_ITERS, BREAKDOWN = 0, 1, 2
W_ODO, W_CLO = (62500.0, 1100.0), (10000.0, 44.0)


def cmul(ar, ai, br, bi):
    """(a + ib)(c + id) = (ac - bd) + i(ad + bc)"""
    return ar * br - ai * bi, ar * bi + ai * br


def cmulc(ar, ai, vr, vi):
    """conj(a) v"""
    return ar * vr + ai * vi, ar * vi - ai * vr


def tree_sum(v):
    """S(v): chunks of 1024 entries, zero-padded, each reduced by the halving tree; the chunk sums, zero-padded to a power
    of two, by the same tree"""
    v = np.asarray(v, dtype=np.float64)
    nch = max(1, (v.size + CHUNK - 1) // CHUNK)
    a = np.zeros(nch * CHUNK, dtype=np.float64)
    a[:v.size] = v
    a = a.reshape(nch, CHUNK)
    h = CHUNK // 2
    while h >= 1:
        a = a[:, :h] + a[:, h:2 * h]
        h //= 2
    P = 1
    while P < nch:
        P *= 2
    b = np.zeros(P, dtype=np.float64)
    b[:nch] = a[:, 0]
    h = P // 2
    while h >= 1:
        b = b[:h] + b[h:2 * h]
        h //= 2
    return float(b[0])


def _fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic; the mutation tests only)"""
    return float(fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c)))


def session_layout(M, starts, segment=SEGMENT):
    """starts (None = one session) -> (starts int64 [S], sess [M], pos [M], seg [M], nseg): the session of every scan, its
    position in the session, the global number of its segment (sessions in order, ceil(len / segment) segments each)"""
    starts = np.zeros(1, np.int64) if starts is None or len(starts) == 0 else np.asarray(starts, dtype=np.int64)
    k = np.arange(M, dtype=np.int64)
    sess = np.searchsorted(starts, k, side="right") - 1
    pos = k - starts[sess] if M else k
    ends = np.append(starts[1:], M)
    lens = np.maximum(ends - starts, 0)
    segbase = np.concatenate(([0], np.cumsum((lens + segment - 1) // segment)))
    seg = segbase[sess] + pos // segment if M else k
    return starts, sess, pos, seg, int(segbase[-1])


class _Problem:
    """Everything both stages share: edges, which scans move, the term table of every free scan."""

    def __init__(self, X, rows, cols, T, starts, fixed, weight, w_odo, w_clo, segment, tail_first):
        M, C = X.shape[0], rows.size
        self.M, self.C, self.segment = M, C, segment
        self.starts, self.sess, self.pos, self.seg, self.nseg = session_layout(M, starts, segment)
        self.g0r, self.g0i, self.t0r, self.t0i = (np.ascontiguousarray(X[:, j]) for j in range(4))
        fixed = (np.arange(M) == 0) if fixed is None else (np.asarray(fixed).reshape(-1) != 0)
        self.fixed = fixed
        # ---- status
        self.status = 0
        with np.errstate(all="ignore"):
            n2 = self.g0r * self.g0r + self.g0i * self.g0i
            if not np.isfinite(X).all() or (n2 == 0.0).any():
                self.status |= NONFINITE
        if not fixed.any():
            self.status |= NO_ANCHOR
        # ---- live closures
        weight = np.ones(C, np.float64) if weight is None else np.asarray(weight, dtype=np.float64).reshape(-1)
        with np.errstate(all="ignore"):
            tn2 = T[:, 0] * T[:, 0] + T[:, 1] * T[:, 1]
            live = ((rows >= 0) & (rows < M) & (cols >= 0) & (cols < M) & (rows != cols) & np.isfinite(T).all(axis=1) &
                    (tn2 > 0.0) & np.isfinite(weight) & (weight > 0.0))
        self.live = live
        if self.status:
            return
        # ---- edges: odometry edge k-1 -> k has the id k, closure p the id M + p
        E = M + C
        tail, head = np.zeros(E, np.int64), np.zeros(E, np.int64)
        zrr, zri, ztr, zti = (np.zeros(E) for _ in range(4))
        zrr[:] = 1.0
        wr, wt = np.zeros(E), np.zeros(E)
        has_in = self.pos > 0
        self.has_in = has_in
        k = np.nonzero(has_in)[0]
        with np.errstate(all="ignore"):
            qr, qi = cmulc(self.g0r[k - 1], self.g0i[k - 1], self.g0r[k], self.g0i[k])
            n = np.sqrt(qr * qr + qi * qi)
            zrr[k], zri[k] = qr / n, qi / n
            ztr[k], zti[k] = cmulc(self.g0r[k - 1], self.g0i[k - 1], self.t0r[k] - self.t0r[k - 1], self.t0i[k] - self.t0i[k - 1])
        tail[k], head[k] = k - 1, k
        wr[k], wt[k] = w_odo[0], w_odo[1]
        p = np.nonzero(live)[0]
        n = np.sqrt(tn2[p])
        zrr[M + p], zri[M + p] = T[p, 0] / n, T[p, 1] / n
        ztr[M + p], zti[M + p] = T[p, 2], T[p, 3]
        tail[M + p], head[M + p] = cols[p], rows[p]
        wr[M + p], wt[M + p] = w_clo[0] * weight[p], w_clo[1] * weight[p]
        self.tail, self.head, self.zrr, self.zri, self.ztr, self.zti, self.wr, self.wt = tail, head, zrr, zri, ztr, zti, wr, wt
        # ---- which scans move
        S = self.starts.size
        anchored = np.zeros(S, bool)
        anchored[self.sess[fixed]] = True
        adj = np.zeros((S, S), bool)
        adj[self.sess[rows[p]], self.sess[cols[p]]] = True
        adj |= adj.T
        active = anchored.copy()
        while True:
            grown = active | adj[active].any(axis=0)
            if (grown == active).all():
                break
            active = grown
        self.active = active
        self.free = active[self.sess] & ~fixed if M else np.zeros(0, bool)
        # ---- the term table of every free scan: (edge, 0 = this scan is the head | 1 = the tail), in the order of the definition
        heads = [[] for _ in range(M)]
        tails = [[] for _ in range(M)]
        for q in p:
            heads[rows[q]].append(M + q)
            tails[cols[q]].append(M + q)
        table = []
        for s in range(M):
            if not self.free[s]:
                table.append([])
                continue
            a = ([(s, 0)] if has_in[s] else []) + [(e, 0) for e in heads[s]]
            b = ([(s + 1, 1)] if s + 1 < M and has_in[s + 1] else []) + [(e, 1) for e in tails[s]]
            table.append(b + a if tail_first else a + b)
        self.tlen = np.array([len(t) for t in table], dtype=np.int64)
        width = int(self.tlen.max()) if M else 0
        self.tedge = np.zeros((M, width), np.int64)
        self.tkind = np.zeros((M, width), np.int64)
        for s, t in enumerate(table):
            for j, (e, kind) in enumerate(t):
                self.tedge[s, j], self.tkind[s, j] = e, kind

    def accumulate(self, head_term, tail_term, parts=2):
        """the sum over every free scan's terms, starting from the first term; head_term / tail_term(k, e) -> parts arrays"""
        acc = [np.zeros(self.M) for _ in range(parts)]
        for j in range(self.tedge.shape[1]):
            for kind, fn in ((0, head_term), (1, tail_term)):
                k = np.nonzero((self.tlen > j) & (self.tkind[:, j] == kind))[0]
                if k.size == 0:
                    continue
                term = fn(k, self.tedge[k, j])
                for a, t in zip(acc, term):
                    a[k] = t if j == 0 else a[k] + t
        return acc


def _stage(pb, rot, ur, ui, gr, gi, max_iters, rel_tol, precond, tree, fused):
    """one preconditioned conjugate-gradient solve -> (ur, ui, iterations, reason, rz0, rz)"""
    M, SEG, free = pb.M, pb.segment, pb.free
    w = pb.wr if rot else pb.wt
    zr, zi = pb.zrr, pb.zri

    def A(xr, xi):
        if rot:
            def head(k, e):
                o = pb.tail[e]
                pr, pi = cmul(zr[e], zi[e], xr[o], xi[o])
                return w[e] * (xr[k] - pr), w[e] * (xi[k] - pi)

            def tail(k, e):
                o = pb.head[e]
                pr, pi = cmul(zr[e], zi[e], xr[k], xi[k])
                dr, di = w[e] * (xr[o] - pr), w[e] * (xi[o] - pi)
                cr, ci = cmulc(zr[e], zi[e], dr, di)
                return -cr, -ci
        else:
            def head(k, e):
                o = pb.tail[e]
                return w[e] * (xr[k] - xr[o]), w[e] * (xi[k] - xi[o])

            def tail(k, e):
                o = pb.head[e]
                return -(w[e] * (xr[o] - xr[k])), -(w[e] * (xi[o] - xi[k]))
        return pb.accumulate(head, tail)

    if rot:
        br, bi = np.zeros(M), np.zeros(M)
    else:
        def bhead(k, e):
            pr, pi = cmul(gr[pb.tail[e]], gi[pb.tail[e]], pb.ztr[e], pb.zti[e])
            return w[e] * pr, w[e] * pi

        def btail(k, e):
            pr, pi = cmul(gr[k], gi[k], pb.ztr[e], pb.zti[e])
            return -(w[e] * pr), -(w[e] * pi)
        br, bi = pb.accumulate(bhead, btail)
    diag, = pb.accumulate(lambda k, e: (w[e],), lambda k, e: (w[e],), parts=1)

    # ---- the preconditioner, position-major: [position in the segment][segment]
    k = np.arange(M)
    slot = (pb.pos % SEG, pb.seg)
    shape = (SEG, max(pb.nseg, 1))
    valid = np.zeros(shape, bool)
    valid[slot] = True
    D = np.ones(shape)
    D[slot] = diag
    cpl = np.zeros(shape, bool)
    lowr, lowi = np.zeros(shape), np.zeros(shape)
    if precond == "segment":
        kk = k[(pb.pos % SEG != 0) & free & np.roll(free, 1)]
        cpl[slot[0][kk], slot[1][kk]] = True
        if rot:
            lowr[slot[0][kk], slot[1][kk]] = -(w[kk] * zr[kk])
            lowi[slot[0][kk], slot[1][kk]] = -(w[kk] * zi[kk])
        else:
            lowr[slot[0][kk], slot[1][kk]] = -w[kk]
    piv, lr, li = D.copy(), np.zeros(shape), np.zeros(shape)
    with np.errstate(all="ignore"):
        for j in range(1, SEG):
            c = cpl[j]
            tr, ti = lowr[j] / piv[j - 1], lowi[j] / piv[j - 1]
            lr[j], li[j] = np.where(c, tr, 0.0), np.where(c, ti, 0.0)
            piv[j] = np.where(c, D[j] - (tr * lowr[j] + ti * lowi[j]), D[j])

    def Minv(rr, ri):
        yr, yi = np.zeros(shape), np.zeros(shape)
        yr[slot], yi[slot] = rr, ri
        with np.errstate(all="ignore"):
            for j in range(1, SEG):
                pr, pi = cmul(lr[j], li[j], yr[j - 1], yi[j - 1])
                yr[j], yi[j] = np.where(cpl[j], yr[j] - pr, yr[j]), np.where(cpl[j], yi[j] - pi, yi[j])
            yr, yi = yr / piv, yi / piv
            for j in range(SEG - 2, -1, -1):
                pr, pi = cmulc(lr[j + 1], li[j + 1], yr[j + 1], yi[j + 1])
                yr[j], yi[j] = np.where(cpl[j + 1], yr[j] - pr, yr[j]), np.where(cpl[j + 1], yi[j] - pi, yi[j])
        return np.where(free, yr[slot], 0.0), np.where(free, yi[slot], 0.0)

    def dot(ar, ai, cr, ci):
        if fused:
            v = np.array([_fma(ar[j], cr[j], ai[j] * ci[j]) for j in range(M)])
        else:
            v = ar * cr + ai * ci
        if tree:
            return tree_sum(v)
        s = 0.0
        for x in v:
            s = s + float(x)
        return s

    ur, ui = ur.copy(), ui.copy()
    ar, ai = A(ur, ui)
    rr, ri = np.where(free, br - ar, 0.0), np.where(free, bi - ai, 0.0)
    zvr, zvi = Minv(rr, ri)
    pr, pi = zvr.copy(), zvi.copy()
    rz0 = rz = dot(rr, ri, zvr, zvi)
    it, reason = 0, None
    while it < max_iters and rz > (rel_tol * rel_tol) * rz0 and rz > 0.0:
        apr, api = A(pr, pi)
        pAp = dot(pr, pi, apr, api)
        if not pAp > 0.0:
            reason = BREAKDOWN
            break
        alpha = rz / pAp
        with np.errstate(all="ignore"):            # (non-free entries are never updated)
            ur, ui = np.where(free, ur + alpha * pr, ur), np.where(free, ui + alpha * pi, ui)
            rr, ri = np.where(free, rr - alpha * apr, 0.0), np.where(free, ri - alpha * api, 0.0)
            zvr, zvi = Minv(rr, ri)
            rzn = dot(rr, ri, zvr, zvi)
            beta = rzn / rz
            pr, pi = np.where(free, zvr + beta * pr, 0.0), np.where(free, zvi + beta * pi, 0.0)
        rz = rzn
        it += 1
    if reason is None:
        reason = STOP_MAX_ITERS if (rz > (rel_tol * rel_tol) * rz0 and rz > 0.0) else CONVERGED
    return ur, ui, it, reason, rz0, rz


def optimize(X, rows, cols, T, starts=None, fixed=None, weight=None, w_odo=W_ODO, w_clo=W_CLO, max_iters=1000,
             rel_tol=1e-9, precond="segment", segment=SEGMENT, tree=True, tail_first=False, fused=False):
    """-> (X_out float64 [M,4], info int32 [8], resid float64 [4]); see include/sgpr_posegraph.h.
    info: status flags, iterations of R and T, stop reason of R and T, live closures, free scans, active sessions."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1, 4))
    rows, cols = np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(cols, dtype=np.int64).reshape(-1)
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4)
    info, resid = np.zeros(8, np.int32), np.zeros(4, np.float64)
    if X.shape[0] == 0:
        return X.copy(), info, resid
    pb = _Problem(X, rows, cols, T, starts, fixed, weight, w_odo, w_clo, segment, tail_first)
    info[0] = pb.status
    if pb.status:
        return X.copy(), info, resid
    info[5], info[6], info[7] = int(pb.live.sum()), int(pb.free.sum()), int(pb.active.sum())
    if info[5] == 0:                       # nothing ties the odometry down: the input, bit for bit
        return X.copy(), info, resid
    free = pb.free
    gr, gi, info[1], info[3], resid[0], resid[1] = _stage(pb, True, pb.g0r, pb.g0i, None, None, max_iters, rel_tol, precond,
                                                          tree, fused)
    with np.errstate(all="ignore"):
        n = np.sqrt(gr * gr + gi * gi)
        bad = free & ~(np.isfinite(n) & (n > 0.0))
        ok = free & ~bad
        gr, gi = np.where(ok, gr / n, pb.g0r), np.where(ok, gi / n, pb.g0i)
    if bad.any():
        info[0] |= DEGENERATE
    tr, ti, info[2], info[4], resid[2], resid[3] = _stage(pb, False, pb.t0r, pb.t0i, gr, gi, max_iters, rel_tol, precond, tree,
                                                          fused)
    out = X.copy()
    out[free] = np.stack((gr, gi, tr, ti), axis=1)[free]
    return out, info, resid


def normal_equations(X, rows, cols, T, starts=None, fixed=None, weight=None, w_odo=W_ODO, w_clo=W_CLO):
    """The two linear systems of the definition, assembled for a direct solve (scipy): a function
    solve(spsolve) -> X_out that solves stage R, normalises, and solves stage T on the free scans.  Complex Hermitian
    systems; the boundary values enter the right-hand sides."""
    import scipy.sparse as sp
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1, 4))
    rows, cols = np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(cols, dtype=np.int64).reshape(-1)
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4)
    pb = _Problem(X, rows, cols, T, starts, fixed, weight, w_odo, w_clo, SEGMENT, False)
    assert pb.status == 0
    M = pb.M
    e = np.concatenate((np.nonzero(pb.has_in)[0], M + np.nonzero(pb.live)[0]))
    free = pb.free
    idx = np.cumsum(free) - 1
    nf = int(free.sum())

    def system(z, w, rhs, u0):
        # E u = rhs, rows = edges: +1 at the head, -z at the tail, weighted by sqrt(w)
        n = e.size
        Eh = sp.csr_matrix((np.ones(n, complex), (np.arange(n), pb.head[e])), shape=(n, M))
        Et = sp.csr_matrix((-z[e], (np.arange(n), pb.tail[e])), shape=(n, M))
        Em = (Eh + Et).tocsc()
        W = sp.diags(w[e])
        Ef, Eb = Em[:, np.nonzero(free)[0]], Em[:, np.nonzero(~free)[0]]
        H = (Ef.conj().T @ W @ Ef).tocsc()
        g = Ef.conj().T @ (W @ (rhs[e] - Eb @ u0[~free]))
        return H, g

    def solve(spsolve):
        out = X.copy()
        if nf == 0 or not pb.live.any():
            return out
        g0, t0 = pb.g0r + 1j * pb.g0i, pb.t0r + 1j * pb.t0i
        H, b = system(pb.zrr + 1j * pb.zri, pb.wr, np.zeros(M + pb.C, complex), g0)
        g = g0.copy()
        g[free] = spsolve(H, b)
        g[free] /= np.abs(g[free])
        rhs = g[pb.tail] * (pb.ztr + 1j * pb.zti)
        H, b = system(np.ones(M + pb.C, complex), pb.wt, rhs, t0)
        t = t0.copy()
        t[free] = spsolve(H, b)
        out[free] = np.stack((g.real, g.imag, t.real, t.imag), axis=1)[free]
        return out
    return solve
