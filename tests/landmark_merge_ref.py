"""NumPy reference of the record-level merge of landmark maps (include/sgpr_landmark_merge.h, sgpr_landmark_merge;
DESIGN.md §36): the header's definition in float64, one rounding per operation (NumPy rounds every ufunc on its own),
integer sums.  Links and components are landmark_ref's - the records are its points.

merge(...) returns a dict with every output of the call.  merge(..., mutant=NAME) is the definition with one rule altered
(MUTANTS): what a subtly wrong kernel would compute; tests/test_landmark_merge_host.py proves that each one changes an
output on a named case of mutant_cases().  hand_cases() are the hand-made cases at the boundaries of the rules; the host
test checks their answers, the GPU test sends every one of both lists through the kernels.

register(...) is the reference composition of SG.register_maps: map B's landmarks as one query scan of
landmark_relocalize_ref.relocalize against map A, composed with the centring shift."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_ref  # noqa: E402

FIX = landmark_ref.FIX            # 2^24
V_CAP = landmark_ref.D2_CAP       # 2^20
MAX_COUNT = 262144                # 2^18
SUM_LIMIT = 274877906944.0        # 2^38
COUNT_TOP = 2 ** 31 - 1
THREADS = 256
RECORD = ("center", "label", "count", "first", "sessions", "spread")

# "old_centres": the spread about the members' old centres, v = spread spread (no parallel-axis term);
# "cap_after": v capped after the multiplication, min(v n, 2^20); "ids_high": landmarks numbered by their HIGHEST member;
# "recompute_singleton": a component of one goes through the formulas instead of being copied; "across_only": links
# between a record of A and one of B only; "float_sum": center' by a float64 sum of p n in member order / sum;
# "strict": d2 < r r; "z_strict": |dz| < tau_z; "unweighted": center' the plain mean of the members' centres;
# "first_of_root": first' of the lowest member, not the lowest first; "null_is_identity": no pose runs the identity pose;
# "no_shift": B's sessions are not shifted; "no_first_base": B's first without first_base; "count_wraps": count' is the
# sum cast to int32 instead of saturating; "keep_after": a record a mask drops still bridges its neighbours
MUTANTS = ("old_centres", "cap_after", "ids_high", "recompute_singleton", "across_only", "float_sum", "strict", "z_strict",
           "unweighted", "first_of_root", "null_is_identity", "no_shift", "no_first_base", "count_wraps", "keep_after")


def workspace_bytes(L_a, L_b):
    """sgpr_landmark_merge_workspace_bytes: per record three [3] float64 / int64 rows, three 64-bit and six 32-bit words;
    the cell table of table_slots(T) slots; a root count per workgroup; one block of counters"""
    T = int(L_a) + int(L_b)
    if L_a < 0 or L_b < 0 or T == 0 or T > 0x7fffffff:
        return 0
    H = 1024
    while H < 2 * T:
        H <<= 1
    B = (T + THREADS - 1) // THREADS

    def al(v):
        return (v + 255) & ~255
    return al(T * 24) * 3 + al(T * 8) * 3 + al(T * 4) * 6 + al(H * 8) + al(H * 4) + al(B * 4) + 256


def lm_of(center, label, count=None, first=None, sessions=None, spread=None):
    """a map dict from lists"""
    n = len(label)
    return {"center": np.array(center, np.float64).reshape(-1, 3), "label": np.array(label, np.int32).reshape(-1),
            "count": np.array([1] * n if count is None else count, np.int32).reshape(-1),
            "first": np.array(list(range(n)) if first is None else first, np.int32).reshape(-1),
            "sessions": np.array([1] * n if sessions is None else sessions, np.uint64).reshape(-1),
            "spread": np.array([0.0] * n if spread is None else spread, np.float64).reshape(-1)}


def _records(lm):
    if lm is None:
        return lm_of(np.zeros((0, 3)), [])
    return {"center": np.array(np.asarray(lm["center"], np.float64).reshape(-1, 3)), "label": np.array(lm["label"], np.int32).reshape(-1),
            "count": np.array(lm["count"], np.int32).reshape(-1), "first": np.array(lm["first"], np.int32).reshape(-1),
            "sessions": np.array(lm["sessions"]).astype(np.uint64).reshape(-1), "spread": np.array(lm["spread"], np.float64).reshape(-1)}


def input_records(a, b=None, pose=None, session_shift=0, first_base=0, mutant=None):
    """INPUT RECORD of every record, A's then B's -> (dict of the six arrays [L_a + L_b], L_a)"""
    ra, rb = _records(a), _records(b)
    c = rb["center"].copy()
    if pose is None and mutant == "null_is_identity":
        pose = (1.0, 0.0, 0.0, 0.0)
    if pose is not None:
        cs, sn, X, Y = (np.float64(v) for v in np.asarray(pose, np.float64).reshape(4))
        x, y = rb["center"][:, 0], rb["center"][:, 1]
        with np.errstate(all="ignore"):
            c[:, 0] = (cs * x - sn * y) + X
            c[:, 1] = (sn * x + cs * y) + Y
    shift = np.uint64(0 if mutant == "no_shift" else session_shift)
    base = 0 if mutant == "no_first_base" else int(first_base)
    rb = dict(rb, center=c, sessions=rb["sessions"] << shift, first=(rb["first"].astype(np.int64) + base).astype(np.int32))
    return {k: np.concatenate((ra[k], rb[k])) for k in RECORD}, ra["label"].size


def _table(radius, n_labels):
    radius = np.atleast_1d(np.asarray(radius, np.float64))
    if n_labels is None:
        n_labels = radius.size if radius.size > 1 else 12
    if radius.size == 1:
        radius = np.full(n_labels, radius[0])
    return radius, n_labels


def eligible(rec, radius):
    """the eligible rule on input records, before the keep masks -> bool [T]"""
    c, lab, cnt, sp = rec["center"], rec["label"].astype(np.int64), rec["count"].astype(np.int64), rec["spread"]
    ok = (lab >= 0) & (lab < radius.size)
    ok[ok] = radius[lab[ok]] > 0
    ok &= (cnt >= 1) & (cnt <= MAX_COUNT)
    with np.errstate(all="ignore"):
        ok &= np.isfinite(c).all(1) & (np.abs(c * cnt.astype(np.float64)[:, None]) <= SUM_LIMIT).all(1)
        ok &= np.isfinite(sp) & (sp >= 0)
    return ok


def merge(a, b=None, keep_a=None, keep_b=None, pose=None, session_shift=0, first_base=0, radius=0.75, tau_z=0.75, n_labels=None,
          max_out=None, mutant=None):
    """a, b: dicts of center f64 [L,3], label, count, first i32 [L], sessions u64 [L], spread f64 [L] (b None: none);
    keep_a, keep_b: u8 [L] or None -> dict: the six records of the merged map, min(L', max_out) rows (None: L'),
    old_to_new i32 [L_a + L_b], num = (L', dropped by a mask, dropped as ineligible, components of several members),
    links (the number of linked pairs)"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutant,))
    rec, L_a = input_records(a, b, pose, session_shift, first_base, mutant)
    T = rec["label"].size
    radius, n_labels = _table(radius, n_labels)
    kept = np.ones(T, bool)
    if keep_a is not None:
        kept[:L_a] = np.asarray(keep_a).reshape(-1) != 0
    if keep_b is not None:
        kept[L_a:] = np.asarray(keep_b).reshape(-1) != 0
    fit = eligible(rec, radius)
    live = kept & fit
    p, lab = rec["center"], rec["label"].astype(np.int64)
    linkable = fit if mutant == "keep_after" else live
    x, y = landmark_ref._links(p, lab, linkable, radius, np.float64(tau_z),
                               "strict" if mutant == "strict" else "z_strict" if mutant == "z_strict" else None)
    if mutant == "across_only":
        cross = (x >= L_a) != (y >= L_a)
        x, y = x[cross], y[cross]
    parent = landmark_ref._components(T, x, y)
    members = np.flatnonzero(live)
    root = parent[members]
    if mutant == "ids_high":
        top = np.zeros(T, np.int64)
        np.maximum.at(top, root, members)
        keys, lid = np.unique(top[root], return_inverse=True)
    else:
        keys, lid = np.unique(root, return_inverse=True)         # roots ascending: ids by the lowest member
    lid = lid.reshape(-1)
    L = keys.size
    old_to_new = np.full(T, -1, np.int32)
    old_to_new[members] = lid
    size = np.bincount(lid, minlength=L)
    lowest = np.full(L, T, np.int64)
    np.minimum.at(lowest, lid, members)
    out = {k: rec[k][lowest].copy() for k in RECORD}             # a component of one: the input record, bit for bit
    fused = np.flatnonzero((size > 1) | (mutant == "recompute_singleton"))
    if fused.size:
        slot = np.full(L, -1, np.int64)
        slot[fused] = np.arange(fused.size)
        sel = slot[lid] >= 0
        mem, row = members[sel], slot[lid[sel]]
        n_i = rec["count"][mem].astype(np.float64)
        total = np.zeros(fused.size, np.int64)
        np.add.at(total, row, rec["count"][mem].astype(np.int64))
        tot = total.astype(np.float64)
        with np.errstate(all="ignore"):
            S = np.zeros((fused.size, 3), np.int64)
            np.add.at(S, row, np.rint((p[mem] * n_i[:, None]) * FIX).astype(np.int64))     # (wraps modulo 2^64)
            centre = S.astype(np.float64) / (tot * FIX)[:, None]
            if mutant == "float_sum":
                acc = np.zeros((fused.size, 3))
                for r, v in zip(row, p[mem] * n_i[:, None]):
                    acc[r] = acc[r] + v
                centre = acc / tot[:, None]
            if mutant == "unweighted":
                S = np.zeros((fused.size, 3), np.int64)
                np.add.at(S, row, np.rint(p[mem] * FIX).astype(np.int64))
                centre = S.astype(np.float64) / (size[fused].astype(np.float64) * FIX)[:, None]
            ax, ay = p[mem, 0] - centre[row, 0], p[mem, 1] - centre[row, 1]
            sp = rec["spread"][mem]
            v = sp * sp if mutant == "old_centres" else sp * sp + (ax * ax + ay * ay)
            term = np.minimum(v * n_i, V_CAP) if mutant == "cap_after" else np.minimum(v, V_CAP) * n_i
            Q = np.zeros(fused.size, np.uint64)
            np.add.at(Q, row, np.rint(term * FIX).astype(np.int64).astype(np.uint64))
            spread = np.sqrt(Q.astype(np.float64) / (tot * FIX))
        bits = np.zeros(fused.size, np.uint64)
        np.bitwise_or.at(bits, row, rec["sessions"][mem])
        first = np.full(fused.size, 2 ** 31 - 1, np.int64)
        np.minimum.at(first, row, rec["first"][mem].astype(np.int64))
        out["center"][fused] = centre
        out["count"][fused] = total.astype(np.int32) if mutant == "count_wraps" else np.minimum(total, COUNT_TOP).astype(np.int32)
        out["sessions"][fused] = bits
        if mutant != "first_of_root":
            out["first"][fused] = first.astype(np.int32)
        out["spread"][fused] = spread
    k = L if max_out is None else min(L, int(max_out))
    res = {key: out[key][:k] for key in RECORD}
    res["old_to_new"] = old_to_new
    res["num"] = np.array([L, int((~kept).sum()), int((kept & ~fit).sum()), int((size > 1).sum())], np.int32)
    res["links"] = int(x.size)
    return res


def remap(node_landmark, old_to_new):
    """landmarks.remap: ids >= 0 through the table, a dropped landmark becomes -2; -1 and -2 stay"""
    node = np.asarray(node_landmark).astype(np.int64)
    table = np.asarray(old_to_new).astype(np.int64)
    out = node.copy()
    hit = node >= 0
    new = table[node[hit]]
    out[hit] = np.where(new >= 0, new, -2)
    return out.astype(np.int32)


def compose(a, b):
    """a o b of sgpr_landmark_track.h on (c, s, x, y)"""
    ac, as_, ax, ay = (np.float64(v) for v in a)
    bc, bs, bx, by = (np.float64(v) for v in b)
    return np.array([ac * bc - as_ * bs, as_ * bc + ac * bs, (ac * bx - as_ * by) + ax, (as_ * bx + ac * by) + ay])


def query_scan(b, use_b=None, min_count=3):
    """map B's selected landmarks as ONE query scan: centres minus their planar mean in float64, then float32
    -> (centers f32 [1,n,3], labels i32 [1,n], shift = the pose (1, 0, -mean_x, -mean_y), the selected ids)"""
    rb = _records(b)
    pick = rb["count"] >= int(min_count)
    if use_b is not None:
        pick &= np.asarray(use_b).reshape(-1) != 0
    ids = np.flatnonzero(pick)
    c = rb["center"][ids]
    mean = c[:, :2].mean(axis=0) if ids.size else np.zeros(2)
    q = c.copy()
    q[:, :2] -= mean
    return q.astype(np.float32)[None], rb["label"][ids][None].astype(np.int32), np.array([1.0, 0.0, -mean[0], -mean[1]]), ids


def register(a, b, use_a=None, use_b=None, min_count=3, ratio=0.7, **kw):
    """the reference composition of SG.register_maps -> (pose (c, s, X, Y) carrying B's frame into A's, or None when the
    scan is not found or is ambiguous at `ratio`; info: found, ambiguous, inliers, inliers_other, hypotheses)"""
    import landmark_relocalize_ref as rref
    ra = _records(a)
    pick = ra["count"] >= int(min_count)
    if use_a is not None:
        pick &= np.asarray(use_a).reshape(-1) != 0
    cen, lab, shift, _ = query_scan(b, use_b, min_count)
    out = rref.relocalize(cen, lab, ra["center"], ra["label"], pick.astype(np.uint8), **kw)
    stat = out["stat"][0]
    found = bool(stat[5] & 1)
    ambiguous = found and stat[1] >= float(ratio) * stat[0]
    info = {"found": found, "ambiguous": bool(ambiguous), "inliers": int(stat[0]), "inliers_other": int(stat[1]),
            "hypotheses": int(out["hyp"][0])}
    if not found or ambiguous:
        return None, info
    return compose(out["poses"][0], shift), info


# ------------------------------------------------------------------ cases
def up(v):
    return np.nextafter(np.float64(v), np.inf)


def down(v):
    return np.nextafter(np.float64(v), -np.inf)


def _case(a, b=None, **kw):
    return {"a": a, "b": b, "kw": kw}


def run(case, **over):
    kw = dict(case["kw"])
    kw.update(over)
    return merge(case["a"], case["b"], **kw)


def chain_case():
    """A - B - A: A's records at x = 0 and 1.5, B's at 0.75 between them; counts 1, 2 (A) and 1 (B)"""
    a = lm_of([(0.0, 0.0, 0.0), (1.5, 0.0, 0.0)], [0, 0], count=[1, 2], first=[7, 3], sessions=[1, 2], spread=[0.0, 0.5])
    b = lm_of([(0.75, 0.0, 0.25)], [0], count=[1], first=[0], sessions=[1], spread=[0.25])
    return _case(a, b, session_shift=2, first_base=100)


def random_case(L_a, L_b, seed, labels=3, dup=0.3, drop=0.1, with_pose=True, keep=True):
    """L_a + L_b made-up records over a square: about `dup` of them lie within the radius of an earlier one (of either
    map), about `drop` are made ineligible in one way or another; B is stored in a displaced frame.
    -> a case (a, b, kw with keep masks, pose, session_shift, first_base)"""
    rng = np.random.default_rng(seed)
    T = L_a + L_b
    extent = max(4.0, 2.0 * np.sqrt(max(T, 1)))
    pts = np.concatenate((rng.uniform(-extent, extent, size=(T, 2)), rng.uniform(-1.0, 1.0, size=(T, 1))), axis=1)
    lab = rng.integers(0, labels, size=T)
    for t in range(1, T):
        if rng.random() < dup:
            o = int(rng.integers(0, t))
            pts[t, :2] = pts[o, :2] + rng.normal(0.0, 0.3, size=2)
            pts[t, 2] = pts[o, 2] + rng.normal(0.0, 0.3)
            lab[t] = lab[o]
    order = rng.permutation(T)
    pts, lab = pts[order], lab[order]
    count = rng.integers(1, 40, size=T)
    spread = rng.uniform(0.0, 0.4, size=T)
    bad = rng.random(T) < drop
    kind = rng.integers(0, 5, size=T)
    count = np.where(bad & (kind == 0), 0, count)
    spread = np.where(bad & (kind == 1), -0.5, spread)
    spread = np.where(bad & (kind == 2), np.nan, spread)
    lab = np.where(bad & (kind == 3), labels + 20, lab)
    pts[bad & (kind == 4), 1] = np.inf
    first = rng.integers(0, 1 << 20, size=T)
    sess = rng.integers(1, 8, size=T)
    yaw, X, Y = 0.9, 300.0, -120.0
    pose = np.array([np.cos(yaw), np.sin(yaw), X, Y]) if with_pose else None
    cb = pts[L_a:].copy()
    if with_pose:                                                 # B's centres in B's frame: inverse(pose) of the points
        dx, dy = cb[:, 0] - X, cb[:, 1] - Y
        cb[:, 0], cb[:, 1] = pose[0] * dx + pose[1] * dy, pose[0] * dy - pose[1] * dx
    a = lm_of(pts[:L_a], lab[:L_a], count[:L_a], first[:L_a], sess[:L_a], spread[:L_a])
    b = lm_of(cb, lab[L_a:], count[L_a:], first[L_a:], sess[L_a:], spread[L_a:]) if L_b else None
    kw = dict(pose=pose if L_b else None, session_shift=3, first_base=1 << 20, n_labels=12)
    if keep:
        kw["keep_a"] = (rng.random(L_a) >= 0.1).astype(np.uint8)
        if L_b:
            kw["keep_b"] = (rng.random(L_b) >= 0.1).astype(np.uint8)
    return _case(a, b, **kw)


def cell_width(r):
    """lm_cell_width of sgpr_map.hpp"""
    return max(np.float64(r) * np.float64(1.001), np.float64(0.5))


def cell_coord(v, w):
    """lm_cell_coord of sgpr_map.hpp"""
    return int(np.floor(np.float64(v) / np.float64(w)))


def _mix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & 0xffffffffffffffff
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & 0xffffffffffffffff
    return k ^ (k >> 33)


def cell_key(label, ix, iy):
    """lm_cell_key of sgpr_map.hpp, in Python integers: the 64-bit key under which the kernels file the cell (label, ix,
    iy).  It is a HASH: two cells may share a key, and then they share a list."""
    m = 0xffffffffffffffff
    k = _mix64(((ix & m) + 0x9e3779b97f4a7c15 * (label + 1)) & m)
    k = _mix64(k ^ (((iy & m) * 0xd6e8feb86659fd93) & m))
    return 0 if k == m else k


# Cells of one label that share a key (found by solving the key for iy: mix64 is a bijection and iy enters multiplied by an
# odd constant, so one trial ix in 2^24 has an |iy| below 2^39).  (label, [(ix, iy), ..]): all cells of a row have ONE key.
COLLIDING_CELLS = ((0, [(5, 7), (46189276, 177134394700), (86870242, -28584481588)]),
                   (1, [(-3, 2), (-30668860, 600188191)]))


def collision_case(radius=0.75):
    """Records in cells whose keys collide, and beside them: in every colliding cell a record A in one corner, B and C
    together in the opposite corner (B - C fuse; A is 0.99 m from them and does not), D on B's spot 2 m higher (out of
    tau_z); in the cell to the left a record half a metre from A (it fuses with A: the shared list is met among its nine
    neighbours); diagonally beyond B one more, 0.85 m off (it stays alone).  The records alternate between map A and map
    B.  Every record's cell is checked to be the one meant."""
    w = cell_width(radius)
    recs = []
    for label, cells in COLLIDING_CELLS:
        assert len({cell_key(label, ix, iy) for ix, iy in cells}) == 1
        for ix, iy in cells:
            x0, y0 = (ix + 0.5) * w, (iy + 0.5) * w
            for dx, dy, z, cx, cy in ((-0.35, -0.35, 0.0, 0, 0), (0.35, 0.35, 0.0, 0, 0), (0.35, 0.30, 0.25, 0, 0), (0.35, 0.35, 2.0, 0, 0),
                                      (-0.85, -0.35, 0.0, -1, 0), (0.95, 0.95, 0.0, 1, 1)):
                x, y = np.float64(x0 + dx), np.float64(y0 + dy)
                assert (cell_coord(x, w), cell_coord(y, w)) == (ix + cx, iy + cy), (label, ix, iy, dx, dy)
                recs.append((x, y, z, label))
    far = [abs(y) > 1e11 for _, y, _, _ in recs]
    count = [1 if f else 1 + i % 3 for i, f in enumerate(far)]      # (|y count| <= 2^38: a count of 1 or 2 out there)
    lm = lm_of([r[:3] for r in recs], [r[3] for r in recs], count=count, first=[1000 - 7 * i for i in range(len(recs))],
               sessions=[1 + i % 3 for i in range(len(recs))], spread=[0.01 * (i % 5) for i in range(len(recs))])
    a = {k: v[0::2] for k, v in lm.items()}
    b = {k: v[1::2] for k, v in lm.items()}
    return _case(a, b, session_shift=2, first_base=5000, radius=radius)


def hand_cases():
    """name -> case: every hand-made case the tests run, on the reference and on the GPU"""
    r = 0.75
    cases = {}
    # the radius met exactly and one double beyond; tau_z likewise
    cases["radius_exact"] = _case(lm_of([(0.0, 0.0, 0.0), (r, 0.0, 0.0)], [0, 0]))
    cases["radius_beyond"] = _case(lm_of([(0.0, 0.0, 0.0), (up(r), 0.0, 0.0)], [0, 0]))
    cases["tau_z_exact"] = _case(lm_of([(0.0, 0.0, 0.0), (0.25, 0.0, 0.75)], [0, 0]), tau_z=0.75)
    cases["tau_z_beyond"] = _case(lm_of([(0.0, 0.0, 0.0), (0.25, 0.0, up(0.75))], [0, 0]), tau_z=0.75)
    cases["two_labels_one_spot"] = _case(lm_of([(1.0, 2.0, 0.0), (1.0, 2.0, 0.0)], [0, 1], count=[2, 3]))
    ch = chain_case()
    cases["chain"] = ch
    cases["chain_middle_dropped"] = _case(ch["a"], ch["b"], keep_b=np.array([0], np.uint8), **ch["kw"])
    cases["b_only_component"] = _case(lm_of([(50.0, 0.0, 0.0)], [1], count=[4], spread=[0.125]),
                                      lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0], count=[1, 3], first=[9, 4], sessions=[1, 2]),
                                      session_shift=1, first_base=10)
    # a singleton is copied bit for bit: -0.0 in centre and spread, any first and sessions (NaN bit patterns among them)
    nan_bits = np.array([0x7ff8dead0000beef], np.uint64)
    cases["singleton_bits"] = _case({"center": np.array([[-0.0, 3.0, -0.0]]), "label": np.array([2], np.int32),
                                     "count": np.array([5], np.int32), "first": np.array([-7], np.int32),
                                     "sessions": nan_bits, "spread": np.array([-0.0])})
    one_b = lm_of([(-0.0, 0.0, 0.0)], [0], count=[2], spread=[0.25])
    far_a = lm_of([(40.0, 0.0, 0.0)], [0])
    cases["pose_null"] = _case(far_a, one_b)
    cases["pose_identity"] = _case(far_a, one_b, pose=(1.0, 0.0, 0.0, 0.0))
    # a pose that moves a B record exactly onto the radius of an A record, and one double off it
    cases["pose_onto_radius"] = _case(lm_of([(0.0, 0.0, 0.0)], [0]), lm_of([(0.25, 0.0, 0.0)], [0]), pose=(1.0, 0.0, 0.5, 0.0))
    cases["pose_off_radius"] = _case(lm_of([(0.0, 0.0, 0.0)], [0]), lm_of([(0.25, 0.0, 0.0)], [0]), pose=(1.0, 0.0, up(0.5), 0.0))
    cases["pose_quarter_turn"] = _case(lm_of([(0.0, 2.0, 0.0)], [0], count=[3]), lm_of([(2.0, 0.5, 0.0)], [0]), pose=(0.0, 1.0, 0.0, 0.0))
    two = lm_of([(0.0, 0.0, 0.0)], [0], sessions=[1]), lm_of([(0.25, 0.0, 0.0)], [0], sessions=[(1 << 63) | 5])
    for s in (0, 1, 63):
        cases["session_shift_%d" % s] = _case(*two, session_shift=s)
    cases["first_base"] = _case(lm_of([(0.0, 0.0, 0.0), (30.0, 0.0, 0.0)], [0, 0], first=[50, 60]),
                                lm_of([(0.25, 0.0, 0.0), (60.0, 0.0, 0.0)], [0, 0], first=[3, 4]), first_base=40)
    for n in (0, 1 << 18, (1 << 18) + 1):
        cases["count_%d" % n] = _case(lm_of([(0.0, 0.0, 0.0), (0.25, 0.0, 0.0)], [0, 0], count=[n, 1]))
    for k in range(3):
        for name, v in (("nan", np.nan), ("inf", np.inf)):
            c = [0.0, 0.0, 0.0]
            c[k] = v
            cases["centre_%s_%d" % (name, k)] = _case(lm_of([tuple(c), (0.25, 0.0, 0.0)], [0, 0]))
    cases["centre_at_2^38"] = _case(lm_of([(2.0 ** 37, 0.0, 0.0), (2.0 ** 37, 0.5, 0.0)], [0, 0], count=[2, 1]))
    cases["centre_past_2^38"] = _case(lm_of([(up(2.0 ** 37), 0.0, 0.0), (2.0 ** 37, 0.5, 0.0)], [0, 0], count=[2, 1]))
    cases["centre_b_posed_past_2^38"] = _case(lm_of([(2.0 ** 38, 0.0, 0.0)], [0]), lm_of([(2.0 ** 38, 0.0, 0.0)], [0]),
                                              pose=(1.0, 0.0, 65536.0, 0.0))
    for name, sp in (("neg_zero", -0.0), ("negative", -1e-300), ("nan", np.nan), ("inf", np.inf), ("huge", 1e200)):
        cases["spread_" + name] = _case(lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0], spread=[sp, 0.0]))
    cases["radius_zero_label"] = _case(lm_of([(0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.2, 0.0, 0.0), (0.3, 0.0, 0.0)], [0, 1, 0, 1]),
                                       radius=[0.75, 0.0, 0.75])
    cases["labels_out_of_range"] = _case(lm_of([(0.0, 0.0, 0.0)] * 4, [-1, 3, 2, 2]), radius=[0.75, 0.75, 0.75])
    grid = lm_of([(3.0 * i, 0.0, 0.0) for i in range(6)], [0] * 6, count=[1, 2, 3, 4, 5, 6])
    for cap in (0, 3, 5, 6):
        cases["max_out_%d" % cap] = _case(grid, max_out=cap)
    big = 1 << 18
    n = (1 << 13) + 2                                             # 2^13 x 2^18 = 2^31: past 2^31 - 1
    # a chain 1/32 m apart: few links each, and the weighted coordinate sum stays inside 64 bits
    sat = lm_of([(0.03125 * i, 0.0, 0.0) for i in range(n)], [0] * n, count=[big] * n, spread=[0.5] * n)
    cases["count_saturates"] = _case(sat)
    cases["l_a_zero"] = _case(lm_of(np.zeros((0, 3)), []), lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0], count=[1, 3]), first_base=5)
    cases["l_b_zero"] = _case(lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0], count=[1, 3]), lm_of(np.zeros((0, 3)), []))
    cases["inf_radius"] = _case(lm_of([(-1e9, 5.0, 0.0), (1e9, 0.0, 0.0), (0.0, 0.0, 9.0)], [0, 0, 0]), radius=[np.inf], tau_z=1.0)
    cases["colliding_cells"] = collision_case()
    cases["all_dropped"] = _case(lm_of([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)], [0, 0], count=[0, 1]), keep_a=np.array([1, 0], np.uint8))
    return cases


def mutant_cases():
    """name -> (case, the mutants that must change an output on it)"""
    ch = chain_case()
    cases = {"chain": (ch, ("old_centres", "unweighted", "first_of_root", "no_shift", "no_first_base")),
             "chain_middle_dropped": (_case(ch["a"], ch["b"], keep_b=np.array([0], np.uint8), **ch["kw"]), ("keep_after",)),
             "radius_exact": (hand_cases()["radius_exact"], ("strict",)),
             "tau_z_exact": (hand_cases()["tau_z_exact"], ("z_strict",)),
             "pose_null": (hand_cases()["pose_null"], ("null_is_identity",)),
             "count_saturates": (hand_cases()["count_saturates"], ("count_wraps",)),
             # v = 9.0625 is far below the cap, v n = 9.0625 x 2^18 far above it
             "heavy_member": (_case(lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0], count=[1 << 18, 1 << 18], spread=[3.0, 3.0])),
                              ("cap_after",)),
             # ids by the highest member: the pair (0, 3) then comes after the singletons 1 and 2
             "interleaved": (_case(lm_of([(0.0, 0.0, 0.0), (10.0, 0.0, 0.0), (20.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0] * 4)), ("ids_high",)),
             # a singleton whose centre does not survive (c n 2^24 rounded) / (n 2^24)
             "odd_singleton": (_case(lm_of([(0.1, 1.0 / 3.0, 0.7)], [0], count=[3], spread=[0.3])), ("recompute_singleton",)),
             "inside_a": (_case(lm_of([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], [0, 0]), lm_of([(30.0, 0.0, 0.0)], [0])), ("across_only",)),
             "random": (random_case(120, 90, 3), tuple(m for m in MUTANTS if m not in ("null_is_identity", "count_wraps", "strict",
                                                                                        "z_strict", "cap_after")))}
    return cases
