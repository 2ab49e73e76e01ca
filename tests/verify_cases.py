"""Named, deterministic cases that put sgpr_verify_pairs ON its rules (include/sgpr.h): every comparison
at its threshold and one float32 away from it, the two tie rules, the cap at every base pair, the refinement fallbacks and
the structural points of the kernel (compaction across waves, 256-candidate chunks, ring flushes).

tests/test_verify_boundary_host.py proves - without a GPU - that each case really sits on its rule: the altered
definitions of geo_ref.verify_pair(mutant=...) give another record, threshold cases flip between their runs, probes open
no hypothesis of their own, the intermediates are exact.  tests/test_gpu_verify_boundary.py runs the SAME data through
the kernel and compares bit for bit.

Boundary cases use coordinates that are exact in binary (integers, halves, quarters) and an identity (or quarter-turn)
winning hypothesis, so every intermediate of the definition is exact.  A *probe* is a node of A that carries the
property under test; it lies closer than min_base to every other node of A, so it is in no base pair.  The rounding
cases hold values found by a search on the CPU (the search is not part of this file; the host test re-derives with
fractions.Fraction that the literals have the stated property)."""
import collections

import numpy as np

f32 = np.float32
INF = float("inf")
DEFAULTS = dict(tau_edge=0.5, tau_in=0.6, tau_z=1.0, min_base=5.0, max_hyp=65536)
NO_HYPOTHESIS, TRUNCATED = 2, 4

Case = collections.namedtuple("Case", "name group n ca la cb lb runs probes exact finite")
# runs: [(tolerances, expected fields)]; probes: slots of A; exact: the winning hypothesis is the identity and every
# intermediate exact (checked with Fractions); finite: inputs finite and no product overflows (flags == 0 must then
# come with a finite coarse transform)


def up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def dn(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def graph(n_slots, nodes):
    """nodes: (slot, x, y, z, label)"""
    c = np.zeros((n_slots, 3), f32)
    lab = -np.ones(n_slots, np.int32)
    for slot, x, y, z, l in nodes:
        assert lab[slot] < 0, "slot used twice"
        c[slot] = (x, y, z)
        lab[slot] = l
    return c, lab


def tol(**kw):
    t = dict(DEFAULTS)
    t.update(kw)
    return t


_CASES = collections.OrderedDict()


def _add(name, group, a, b, runs, probes=(), exact=False, finite=True):
    assert name not in _CASES and len(a[1]) == len(b[1])
    _CASES[name] = Case(name, group, len(a[1]), a[0], a[1], b[0], b[1], runs, tuple(probes), exact, finite)


# ---------------------------------------------------------------------------------------------- the enumeration order
def enumerate_hypotheses(case, t):
    """The admissible hypotheses of a case in the order of the definition's cap (base pairs ascending) and, inside a base
    pair, of the kernel's candidate index (j over the range of la[i], j' over the range of la[i'], B ranked by (label,
    slot)) - independent of geo_ref's vectorised enumeration.  The cap is ignored.
    Returns (hyps [(i, i', j, j') slots], pairs [(i, i', candidates, admissible, admissible per 256-candidate chunk)])."""
    ca, la, cb, lb = case.ca, case.la, case.cb, case.lb
    ra = [int(s) for s in np.flatnonzero(la >= 0)]
    rb = np.flatnonzero(lb >= 0)
    order = rb[np.argsort(lb[rb], kind="stable")]
    rng = {p: order[lb[order] == la[p]] for p in ra}
    tau_edge, min_base = f32(t["tau_edge"]), f32(t["min_base"])
    hyps, pairs = [], []
    with np.errstate(all="ignore"):
        for n, i in enumerate(ra):
            for i2 in ra[n + 1:]:
                ux, uy = ca[i2, 0] - ca[i, 0], ca[i2, 1] - ca[i, 1]
                lu = np.sqrt(ux * ux + uy * uy)
                js, j2s = rng[i], rng[i2]
                total = len(js) * len(j2s)
                if not lu >= min_base or total == 0:
                    pairs.append((i, i2, total, 0, ()))
                    continue
                J, J2 = np.repeat(js, len(j2s)), np.tile(j2s, len(js))
                vx, vy = cb[J2, 0] - cb[J, 0], cb[J2, 1] - cb[J, 1]
                lv = np.sqrt(vx * vx + vy * vy)
                adm = (J != J2) & (lu * lv > 0) & (np.abs(lu - lv) <= tau_edge)
                hyps += [(i, i2, int(j), int(j2)) for j, j2 in zip(J[adm], J2[adm])]
                pairs.append((i, i2, total, int(adm.sum()), tuple(int(adm[c:c + 256].sum()) for c in range(0, total, 256))))
    return hyps, pairs


def ring_trace(pairs):
    """The kernel's ring of pending hypotheses, replayed from the per-chunk admissible counts: entries are appended chunk
    by chunk and 256 are evaluated whenever at least 256 are pending.  Returns (pending counts at each in-loop flush,
    entries left for the final flush)."""
    pending, flushes = 0, []
    for p in pairs:
        for c in p[4]:
            pending += c
            if pending >= 256:
                flushes.append(pending)
                pending -= 256
    return flushes, pending


def cap_table(case, t):
    """C_k: the number of hypotheses evaluated before base pair k (k = 0 .. number of base pairs; the last entry is the
    total H)."""
    _, pairs = enumerate_hypotheses(case, t)
    return [0] + list(np.cumsum([p[3] for p in pairs]))


def cap_expect(table, max_hyp):
    """(hypotheses, flags) of the definition for a C_k table: enumeration stops before the first base pair k that starts
    with C_k >= max_hyp."""
    for c in table[:-1]:
        if c >= max_hyp:
            return int(c), TRUNCATED
    return int(table[-1]), 0


# ------------------------------------------------------------------------------------------------------ 1. comparisons
# the identity hypothesis: base pair (0,0)-(5,0), label 1, in slots 1 and 4 of both graphs; probe label 2 in slot 6
_BASE = [(1, 0, 0, 0, 1), (4, 5, 0, 0, 1)]


def _probe_case(name, group, probe, partners, runs, exact=True, n=8):
    a = graph(n, _BASE + [(6,) + tuple(probe) + (2,)])
    b = graph(n, _BASE + [(s,) + tuple(p) + (2,) for s, p in partners])
    _add(name, group, a, b, runs, probes=(6,), exact=exact)


_add("min_base_3_4_5", "comparisons",
     graph(8, [(2, 0, 0, 0, 1), (5, 3, 4, 0, 1)]), graph(8, [(0, 0, 0, 0, 1), (7, 3, 4, 0, 1)]),
     [(tol(min_base=5.0), dict(flags=0, hypotheses=2, inliers=2, base=[2, 5, 0, 7])),
      (tol(min_base=up(5.0)), dict(flags=NO_HYPOTHESIS, hypotheses=0))], exact=True)
_add("tau_edge_8_8p5", "comparisons",
     graph(8, [(0, 0, 0, 0, 1), (3, 8, 0, 0, 1)]), graph(8, [(1, 0, 0, 0, 1), (2, 8.5, 0, 0, 1)]),
     [(tol(tau_edge=0.5), dict(flags=0, hypotheses=2)),
      (tol(tau_edge=dn(0.5)), dict(flags=NO_HYPOTHESIS, hypotheses=0))])
_probe_case("tau_in_quarter", "comparisons", (2, 2, 0), [(6, (2, 2.5, 0))],
            [(tol(tau_in=0.5), dict(flags=0, hypotheses=2, inliers=3, base=[1, 4, 1, 4])),
             (tol(tau_in=dn(0.5)), dict(flags=0, hypotheses=2, inliers=2, base=[1, 4, 1, 4]))])
_probe_case("tau_z_one", "comparisons", (2, 2, 0), [(6, (2, 2, 1.0))],
            [(tol(tau_z=1.0), dict(flags=0, hypotheses=2, inliers=3, base=[1, 4, 1, 4])),
             (tol(tau_z=dn(1.0)), dict(flags=0, hypotheses=2, inliers=2, base=[1, 4, 1, 4]))])
# lv > 0 (now den > 0): B's slots 0 and 1 coincide, slot 2 is the alternative; lu = 0.25 <= tau_edge, so a zero lv
# would pass the length test.  Ordered (j, j') with lv > 0: (0,2) (1,2) (2,0) (2,1)
_add("lv_zero_duplicates", "comparisons",
     graph(8, [(0, 0, 0, 0, 3), (1, 0.25, 0, 0, 3)]),
     graph(8, [(0, 0, 0, 0, 3), (1, 0, 0, 0, 3), (2, 0.25, 0, 0, 3)]),
     [(tol(min_base=0.0), dict(flags=0, hypotheses=4, inliers=2, base=[0, 1, 0, 2]))])

# ------------------------------------------------------------------------------------------------------ 2. rounding
# inlier distance: dx, dy multiples of 2^-22 in [0.25, 0.5): the partner 2 - d is exact and 2 - (2 - d) == d.
# (dx, dy, tau_in): separately rounded dx dx + dy dy == tin2 < either fused form ...
_SEP_IN = (0.3232419490814209, 0.27896618843078613, 0.4269748032093048)
# ... and: either fused form == tin2 < the separately rounded sum
_FUSED_IN = (0.3901069164276123, 0.3490638732910156, 0.5234777927398682)
_probe_case("round_inlier_separate_in", "rounding", (2, 2, 0), [(6, (2 - _SEP_IN[0], 2 - _SEP_IN[1], 0))],
            [(tol(tau_in=_SEP_IN[2]), dict(flags=0, inliers=3, base=[1, 4, 1, 4]))], exact=False)
_probe_case("round_inlier_fused_in", "rounding", (2, 2, 0), [(6, (2 - _FUSED_IN[0], 2 - _FUSED_IN[1], 0))],
            [(tol(tau_in=_FUSED_IN[2]), dict(flags=0, inliers=2, base=[1, 4, 1, 4]))], exact=False)
# base length: (ux, uy, lu rounded separately, lu with either product fused)
_SEP_LONGER = (5.77191162109375, 5.10594367980957, 7.706207275390625, 7.706206798553467)
_FUSED_LONGER = (5.450584411621094, 5.008180618286133, 7.402076721191406, 7.4020771980285645)
for _name, _v, _mb, _e in (("round_base_separate_longer", _SEP_LONGER, _SEP_LONGER[2], dict(flags=0, hypotheses=2)),
                           ("round_base_fused_longer", _FUSED_LONGER, _FUSED_LONGER[3],
                            dict(flags=NO_HYPOTHESIS, hypotheses=0))):
    _g = graph(8, [(0, 0, 0, 0, 1), (5, _v[0], _v[1], 0, 1)])
    _add(_name, "rounding", _g, _g, [(tol(min_base=_mb), _e)])
# subnormals: d2 and tin2 are both subnormal; a kernel that flushes them counts the probe in both runs
_add("subnormal_inlier", "rounding",
     graph(8, [(0, 0, 0, 0, 1), (1, 8e-20, 0, 0, 1), (2, 4e-20, 4e-20, 0, 2)]),
     graph(8, [(0, 0, 0, 0, 1), (1, 8e-20, 0, 0, 1), (2, 4e-20, 4e-20 + 1e-21, 0, 2)]),
     [(tol(tau_edge=0.0, min_base=0.0, tau_in=1e-21), dict(flags=0, hypotheses=2, inliers=3, base=[0, 1, 0, 1])),
      (tol(tau_edge=0.0, min_base=0.0, tau_in=5e-22), dict(flags=0, hypotheses=2, inliers=2, base=[0, 1, 0, 1]))])

# ------------------------------------------------------------------------------------------------------ 3. ties
# a 5 x 5 lattice against itself: the four rotations of the square reach 25 inliers from every base pair
_LATTICE = graph(32, [(5 * r + c, c, r, 0, 1) for r in range(5) for c in range(5)])
LATTICE_TOL = tol(tau_edge=0.0, tau_in=0.25, min_base=1.0)
_add("tie_lattice", "ties", _LATTICE, _LATTICE, [(LATTICE_TOL, dict(flags=0, inliers=25, base=[0, 1, 0, 1]))])
# q(p): base (2,2)-(7,2), the probe (4,4) is 0.25 from two nodes of B; slots 3 and 5 exchanged between the cases.  The
# refined translation in y follows the matched node: down for the one at y = 3.75, up for the one at 4.25
_QBASE = [(1, 2, 2, 0, 1), (4, 7, 2, 0, 1)]
for _name, _lo, _hi, _sign in (("tie_match_low_first", 3.75, 4.25, -1.0), ("tie_match_high_first", 4.25, 3.75, 1.0)):
    _add(_name, "ties", graph(8, _QBASE + [(6, 4, 4, 0, 2)]),
         graph(8, _QBASE + [(3, 4, _lo, 0, 2), (5, 4, _hi, 0, 2)]),
         [(tol(), dict(flags=0, hypotheses=2, inliers=3, base=[1, 4, 1, 4], refined3_sign=_sign))], probes=(6,))

# ------------------------------------------------------------------------------------------------------ 4. the cap
# 12 nodes of one label on distinct integer positions, against itself: 66 base pairs.  Nodes 3 and 4 are closer than
# min_base (a base pair that contributes nothing); in the _tail variant the last two nodes are, so the last base pair is
# inadmissible.
_CAP_XY = [(0, 0), (7, 1), (3, 9), (12, 4), (10, 6), (9, -8), (-6, -7), (15, 11), (2, -12), (-11, 2), (6, 14), (-3, 13)]
_CAP_TAIL_XY = _CAP_XY[:11] + [(4, 13)]
_CAP = graph(16, [(s + 2, x, y, 0, 4) for s, (x, y) in enumerate(_CAP_XY)])
_CAP_TAIL = graph(16, [(s + 2, x, y, 0, 4) for s, (x, y) in enumerate(_CAP_TAIL_XY)])
CAP_KS = (0, 1, 2, 5, 11, 24, 30, 31, 40, 53, 64, 65)      # base pairs whose C_k and C_k + 1 are run (30: nodes 3, 4)
CAP_ZERO_K = 30


def cap_runs(case_graph, ks):
    """[(max_hyp, hypotheses, flags)] for max_hyp = C_k and C_k + 1 at the given k, H - 1 and H (max_hyp >= 1 only)."""
    probe = Case("cap", "cap", 16, case_graph[0], case_graph[1], case_graph[0], case_graph[1], [], (), False, True)
    table = cap_table(probe, tol())
    caps = sorted({int(table[k]) + d for k in ks for d in (0, 1)} | {int(table[-1]) - 1, int(table[-1])})
    return [(m,) + cap_expect(table, m) for m in caps if m >= 1]


_add("cap_12_nodes", "cap", _CAP, _CAP,
     [(tol(max_hyp=m), dict(hypotheses=h, flags=f)) for m, h, f in cap_runs(_CAP, CAP_KS)])
# the cap is reached by the last admissible base pair and only an inadmissible one is left: TRUNCATED, by the definition
_add("cap_12_nodes_short_tail", "cap", _CAP_TAIL, _CAP_TAIL,
     [(tol(max_hyp=m), dict(hypotheses=h, flags=f)) for m, h, f in cap_runs(_CAP_TAIL, (65,))])

# ------------------------------------------------------------------------------------------------ 5. refinement fallbacks
# lu = 8, lv = 8.5: the midpoints coincide, both base nodes land 0.25 from their partners; tau_in = 0.125 misses them
_FB_A, _FB_B = [(0, 0, 0, 0, 1), (3, 8, 0, 0, 1)], [(1, 0, 0, 0, 1), (2, 8.5, 0, 0, 1)]
_add("refine_no_inlier", "fallbacks", graph(8, _FB_A), graph(8, _FB_B),
     [(tol(tau_in=0.125), dict(flags=0, hypotheses=2, inliers=0, inliers_refined=0, refined_is_coarse=True, rmse_nan=True))])
_add("refine_one_inlier", "fallbacks", graph(8, _FB_A + [(5, 4, 0, 0, 2)]), graph(8, _FB_B + [(6, 4.25, 0, 0, 2)]),
     [(tol(tau_in=0.125), dict(flags=0, hypotheses=2, inliers=1, refined_is_coarse=True, rmse=0.0))], probes=(5,))
# two inliers, but the matched nodes of A coincide: D = X = 0
_add("refine_nrm_zero", "fallbacks", graph(8, _FB_A + [(5, 4, 0, 0, 2), (6, 4, 0, 0, 2)]),
     graph(8, _FB_B + [(6, 4.25, 0, 0, 2)]),
     [(tol(tau_in=0.125), dict(flags=0, hypotheses=2, inliers=2, refined_is_coarse=True, rmse=0.0))], probes=(5, 6))

# ------------------------------------------------------------------------------------------------------ 6. the fix
# a base pair of two coincident nodes (lu = 0, legal at min_base = 0) used to be admissible: den = 0, c = s = 0 / 0
_NAN_A, _NAN_B = [(0, 1, 1, 0, 3), (1, 1, 1, 0, 3)], [(2, 0, 0, 0, 3), (5, 0.25, 0, 0, 3)]
_add("nan_hypothesis_alone", "fix", graph(8, _NAN_A), graph(8, _NAN_B),
     [(tol(min_base=0.0), dict(flags=NO_HYPOTHESIS, hypotheses=0))])
# ... and used to win on its slot key over finite hypotheses without inliers (label 7, z offset 9)
_add("nan_hypothesis_beside_finite", "fix",
     graph(8, _NAN_A + [(4, 50, 50, 0, 7), (6, 60, 50, 0, 7)]), graph(8, _NAN_B + [(6, 0, 0, 9, 7), (7, 10, 0, 9, 7)]),
     [(tol(min_base=0.0), dict(flags=0, hypotheses=2, inliers=0, base=[4, 6, 6, 7]))])
# both lengths positive, their float32 product underflows to zero
_UF = graph(8, [(0, 0, 0, 0, 1), (1, 1e-23, 0, 0, 1)])
_add("den_underflow", "fix", _UF, _UF, [(tol(min_base=0.0), dict(flags=NO_HYPOTHESIS, hypotheses=0))])

# ------------------------------------------------------------------------------------------------------ 7. structure
# (compared with the reference only; coordinates are seeded random float32)


def _random_nodes(rng, slots, labels, box):
    slots = list(slots)
    xy = rng.uniform(-box, box, (len(slots), 2))
    z = rng.uniform(-2, 1, len(slots))
    lab = rng.choice(np.asarray(labels), len(slots))
    return [(s, x, y, zz, l) for s, (x, y), zz, l in zip(slots, xy, z, lab)]


def _moved(rng, g, n_slots, yaw=0.7, t=(3.0, -2.0), noise=0.05):
    """The graph rotated, translated, jittered, in permuted slots of an n_slots graph."""
    c, lab = g
    real = np.flatnonzero(lab >= 0)
    slots = rng.permutation(n_slots)[:real.size]
    cs, sn = np.cos(yaw), np.sin(yaw)
    x, y = c[real, 0].astype(np.float64), c[real, 1].astype(np.float64)
    return graph(n_slots, [(s, cs * xx - sn * yy + t[0] + e0, sn * xx + cs * yy + t[1] + e1, zz, l)
                           for s, xx, yy, zz, l, e0, e1 in zip(slots, x, y, c[real, 2], lab[real], rng.normal(0, noise, real.size),
                                  rng.normal(0, noise, real.size))])


def wave_hole_slots(n_a):
    """n_a real slots of 256, spread over all four waves, none within two slots of a wave end."""
    free = [s for s in range(256) if 2 <= s % 64 < 62]
    return [free[k] for k in np.linspace(0, len(free) - 1, n_a).round().astype(int)]


def _structure_compaction():
    rng = np.random.default_rng(1905)
    a = graph(256, _random_nodes(rng, range(192, 256), np.arange(8), 60.0))
    _add("compact_last_wave_only", "structure", a, _moved(rng, a, 256), [(tol(), {})])
    a = graph(256, [(0, -4, 1, 0, 2), (255, 5, 1, 0.5, 2)])
    _add("compact_slots_0_and_255", "structure", a, graph(256, [(255, 0, 0, 0, 2), (128, 9, 0, 0, 2)]),
         [(tol(), dict(flags=0, hypotheses=2, inliers=2))])
    for n_a in (63, 64, 65, 129):
        a = graph(256, _random_nodes(rng, wave_hole_slots(n_a), np.arange(16), 60.0))
        _add("compact_holes_%d" % n_a, "structure", a, _moved(rng, a, 256), [(tol(), {})])


def _structure_chunks():
    rng = np.random.default_rng(1906)
    for n1, n2 in ((15, 17), (16, 16), (16, 17)):
        a = graph(64, [(s, x, y, 0, l) for s, (x, y, l) in
                       enumerate([(0, 0, 1), (9, 2, 2), (-3, 11, 1), (14, 14, 2)])])
        lab = [1] * n1 + [2] * n2
        slots = rng.permutation(64)[:n1 + n2]
        xy = rng.uniform(-12, 12, (n1 + n2, 2))
        b = graph(64, [(s, x, y, 0, l) for s, (x, y), l in zip(slots, xy, lab)])
        _add("chunk_ranges_%d_%d" % (n1, n2), "structure", a, b, [(tol(tau_edge=2.0), {})])


def product_case(name, sizes, n_slots, seed):
    """A has one node per label, B has sizes[l] nodes of label l at distinct places: with a huge finite tau_edge every
    candidate is admissible, so the base pair of labels (l, m) adds exactly sizes[l] * sizes[m] hypotheses."""
    rng = np.random.default_rng(seed)
    a = graph(n_slots, [(3 * l, 20.0 * l, 7.0 * l * l, 0, l + 1) for l in range(len(sizes))])
    lab = np.concatenate([[l + 1] * n for l, n in enumerate(sizes)])
    slots = rng.permutation(n_slots)[:len(lab)]
    xy = rng.uniform(-30, 30, (len(lab), 2))
    b = graph(n_slots, [(s, x, y, 0, l) for s, (x, y), l in zip(slots, xy, lab)])
    total = sum(sizes[l] * sizes[m] for l in range(len(sizes)) for m in range(l + 1, len(sizes)))
    _add(name, "structure", a, b, [(tol(tau_edge=1e6), dict(flags=0, hypotheses=total))])


# name -> (sizes, slots): admissible totals 1, 255, 256 (one full chunk of one base pair), 1280 = 5 x 256 from chunks of
# 200 + 360 + 720 candidates (the ring wraps, the final flush is empty), 1310 (a partial final flush)
PRODUCT_CASES = collections.OrderedDict([
    ("flush_total_1", ((1, 1), 8)), ("flush_total_255", ((15, 17), 64)), ("flush_total_256", ((16, 16), 64)),
    ("flush_total_1280", ((10, 20, 36), 128)), ("flush_total_1310", ((10, 20, 37), 128))])


def _structure_flush():
    for k, (name, (sizes, n_slots)) in enumerate(PRODUCT_CASES.items()):
        product_case(name, sizes, n_slots, 1907 + k)


def _structure_tolerance_ends():
    _add("tolerances_all_zero", "structure", _CAP, _CAP,
         [(tol(tau_edge=0.0, tau_in=0.0, tau_z=0.0), dict(flags=0, inliers=12, inliers_refined=12, base=[2, 3, 2, 3]))])
    rng = np.random.default_rng(1912)
    a = graph(8, _random_nodes(rng, [0, 2, 3, 5, 6, 7], [1, 2], 10.0))
    b = graph(8, _random_nodes(rng, [1, 2, 3, 4, 6, 7], [1, 2], 10.0))
    _add("tolerances_all_inf", "structure", a, b, [(tol(tau_edge=INF, tau_in=INF, tau_z=INF), dict(flags=0, inliers=6))])
    # finite coordinates whose differences and squares overflow float32: the input check passes, lengths become +inf,
    # |inf - inf| is NaN (inadmissible) and a finite lu against lv = +inf is admissible at tau_edge = +inf with den = +inf.
    # What the definition then says is pinned here, not promised to be useful (include/sgpr.h).
    big = [(0, 3e38, 0, 0, 1), (1, 0, 3e38, 0, 1), (2, 0, 0, 0, 1), (3, 1, 1, 0, 1), (4, -3e38, -3e38, 0, 1)]
    _add("overflowing_coordinates", "structure", graph(8, big), graph(8, big),
         [(tol(tau_edge=INF, tau_in=INF, tau_z=INF), {})], finite=False)


_structure_compaction()
_structure_chunks()
_structure_flush()
_structure_tolerance_ends()

CASES = _CASES
GROUPS = collections.OrderedDict()
for _c in CASES.values():
    GROUPS.setdefault(_c.group, []).append(_c.name)

# mutant (geo_ref.MUTANTS) -> the cases whose record under that altered rule differs from the definition's in at least
# one run (asserted by tests/test_verify_boundary_host.py)
MUTANT_CASES = {
    "min_base_strict": ["min_base_3_4_5"],
    "edge_strict": ["tau_edge_8_8p5"],
    "inlier_strict": ["tau_in_quarter"],
    "z_strict": ["tau_z_one"],
    "inlier_fused": ["round_inlier_separate_in", "round_inlier_fused_in"],
    "base_len_fused": ["round_base_separate_longer", "round_base_fused_longer"],
    "flush_subnormals": ["subnormal_inlier"],
    "best_tie_highest": ["tie_lattice"],
    "match_tie_last": ["tie_match_low_first", "tie_match_high_first"],
    "cap_after": ["cap_12_nodes"],
    "cap_strict": ["cap_12_nodes", "cap_12_nodes_short_tail"],
    "lv_zero_ok": ["lv_zero_duplicates", "nan_hypothesis_alone", "nan_hypothesis_beside_finite", "den_underflow"],
}


def mutant_table():
    return "\n".join("  %-18s -> %s" % (m, ", ".join(c)) for m, c in MUTANT_CASES.items())


def check_expect(name, n_run, rec, expect):
    """Assert the fields a case states for a run on one record (reference or kernel)."""
    where = "%s run %d: %s" % (name, n_run, rec)
    for k, v in expect.items():
        if k == "refined_is_coarse":
            assert np.array_equal(rec["refined"], rec["coarse"].astype(np.float64), equal_nan=True), where
        elif k == "rmse_nan":
            assert np.isnan(rec["rmse"]), where
        elif k == "refined3_sign":
            assert np.sign(rec["refined"][3]) == v and abs(rec["refined"][3]) > 0.05, where
        elif k == "base":
            assert rec["base"].tolist() == v, where
        else:
            assert rec[k] == v, (k, v, where)
