"""No GPU: the cases of tests/verify_cases.py really sit on the rules of sgpr_verify_pairs they are named for, so
tests/test_gpu_verify_boundary.py (the same data through the kernel, bit for bit) is sensitive to each of them.

- every altered definition geo_ref.verify_pair(mutant=...) gives another record on the cases listed for it;
- every threshold case flips between its two runs under the definition;
- the preconditions hold: probes are closer than min_base to every other node of A and are in no hypothesis, the
  thresholded quantities are exact (fractions.Fraction), the rounding literals separate the rounded from the fused form,
  the tied hypotheses of the lattice lie in different evaluation batches and waves, the C_k table of the cap cases, the
  candidate and hypothesis totals and the ring's flush points of the structural cases."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_ref  # noqa: E402
import verify_cases as vc  # noqa: E402

f32 = np.float32
_REF = {}


def ref(name, n_run, mutant=None):
    """The reference record of one run of a case (computed once)."""
    key = (name, n_run, mutant)
    if key not in _REF:
        c = vc.CASES[name]
        _REF[key] = geo_ref.verify_pair(c.ca, c.la, c.cb, c.lb, mutant=mutant, **c.runs[n_run][0])
    return _REF[key]


def same(x, y):
    return geo_ref.equal_records(np.array([x]), np.array([y])) == []


def fr(x):
    return Fr(float(f32(x)))


def round32(q):
    """A Fraction rounded once to the nearest float32 (no tie occurs in the cases below: asserted)."""
    x = f32(float(q))
    cands = [x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))]
    err = sorted((abs(Fr(float(c)) - q), float(c)) for c in cands)
    assert err[0][0] < err[1][0], "a tie"
    return f32(err[0][1])


# ------------------------------------------------------------------------------------------------ the reference itself
def test_mutant_names_and_default_path():
    assert set(vc.MUTANT_CASES) == set(geo_ref.MUTANTS) and len(geo_ref.MUTANTS) == 12
    with pytest.raises(ValueError):
        geo_ref.verify_pair(*[getattr(vc.CASES["tau_in_quarter"], k) for k in ("ca", "la", "cb", "lb")], mutant="nothing")
    # the mutants change nothing off the rules: a random pair gives the definition's record under all of them but the
    # two fused sums (which may move a last bit of a length)
    from sg_pr_amd import synth
    centers, labels, _, _ = synth.world_sequence(90, 100, seed=3)          # (60, 0) is a revisit
    centers, labels = centers[[60, 0, 0]], labels[[60, 0, 0]]
    want = geo_ref.verify_pair(centers[0], labels[0], centers[2], labels[2])
    assert want["flags"] == 0 and want["inliers"] > 5
    for m in geo_ref.MUTANTS:
        if m in ("inlier_fused", "base_len_fused", "best_tie_highest", "match_tie_last"):
            continue
        assert same(geo_ref.verify_pair(centers[0], labels[0], centers[2], labels[2], mutant=m), want), m


def test_every_run_gives_what_its_case_states():
    for c in vc.CASES.values():
        assert c.n in (8, 16, 32, 64, 128, 256) and c.runs
        for n, (t, expect) in enumerate(c.runs):
            r = ref(c.name, n)
            vc.check_expect(c.name, n, r, expect)
            if c.finite and r["flags"] == 0:               # no NaN closure edge behind "evaluated, no flag"
                assert np.isfinite(r["coarse"]).all() and np.isfinite(r["refined"]).all(), (c.name, n, r)
            assert r["hypotheses"] < 100000


def test_the_overflowing_case_is_pinned():
    """3e38 coordinates pass the input check; differences and squares overflow.  lu = lv = +inf is inadmissible (|inf - inf|
    is NaN), a finite lu beside lv = +inf is admissible at tau_edge = +inf and has den = +inf: c = s = -0, a "rotation" of
    norm 0.  include/sgpr.h says so; the record is pinned, the rule is not extended."""
    r = ref("overflowing_coordinates", 0)
    assert r["flags"] == 0 and r["hypotheses"] == 18 and r["inliers"] == 5 and r["base"].tolist() == [0, 2, 2, 3]
    assert r["coarse"].tolist() == [0.0, 0.0, 0.5, 0.5] and np.signbit(r["coarse"][:2]).all()


# ------------------------------------------------------------------------------------------------ mutants and flips
@pytest.mark.parametrize("mutant", geo_ref.MUTANTS)
def test_every_mutant_changes_the_record_of_its_cases(mutant):
    for name in vc.MUTANT_CASES[mutant]:
        runs = range(len(vc.CASES[name].runs))
        assert any(not same(ref(name, n), ref(name, n, mutant)) for n in runs), (mutant, name)


def test_threshold_cases_flip_between_their_runs():
    for name in ("min_base_3_4_5", "tau_edge_8_8p5", "tau_in_quarter", "tau_z_one", "subnormal_inlier"):
        c = vc.CASES[name]
        assert len(c.runs) == 2 and not same(ref(name, 0), ref(name, 1)), name
        (t0, _), (t1, _) = c.runs
        moved = [k for k in t0 if t0[k] != t1[k]]
        assert len(moved) == 1, name
        if name != "subnormal_inlier":                     # one float32 apart
            k = moved[0]
            assert f32(t1[k]) in (np.nextafter(f32(t0[k]), f32(np.inf)), np.nextafter(f32(t0[k]), f32(-np.inf))), name
    # the two q(p) cases differ in nothing but which slot holds which of the two equidistant nodes
    a, b = vc.CASES["tie_match_low_first"], vc.CASES["tie_match_high_first"]
    assert np.array_equal(a.ca, b.ca) and np.array_equal(a.cb[[3, 5]], b.cb[[5, 3]]) and np.array_equal(a.lb, b.lb)
    assert ref(a.name, 0)["refined"][3] < 0 < ref(b.name, 0)["refined"][3]


# ------------------------------------------------------------------------------------------------ preconditions
def test_probes_open_no_hypothesis():
    n_probed = 0
    for c in vc.CASES.values():
        for t, _ in c.runs:
            hyps, _ = vc.enumerate_hypotheses(c, t)
            for p in c.probes:
                n_probed += 1
                for o in np.flatnonzero(c.la >= 0):
                    if o != p:
                        ux, uy = c.ca[o, 0] - c.ca[p, 0], c.ca[o, 1] - c.ca[p, 1]
                        assert np.sqrt(ux * ux + uy * uy) < f32(t["min_base"]), (c.name, p, o)
                assert all(p not in h[:2] for h in hyps), c.name
    assert n_probed >= 10


def _identity_is_exact(c, i, i2, j, j2):
    """Fractions: u == v, lu a float32, so den = lu lu = u.u exactly, c = 1, s = 0, and the translation 0."""
    ux, uy = fr(c.ca[i2, 0]) - fr(c.ca[i, 0]), fr(c.ca[i2, 1]) - fr(c.ca[i, 1])
    vx, vy = fr(c.cb[j2, 0]) - fr(c.cb[j, 0]), fr(c.cb[j2, 1]) - fr(c.cb[j, 1])
    assert (ux, uy) == (vx, vy) and fr(c.ca[i, 0]) == fr(c.cb[j, 0]) and fr(c.ca[i, 1]) == fr(c.cb[j, 1])
    lu = f32(np.sqrt(f32(float(ux * ux + uy * uy))))
    assert fr(lu) ** 2 == ux * ux + uy * uy
    return fr(lu)


def test_thresholded_quantities_are_exact():
    c = vc.CASES["min_base_3_4_5"]
    lu = _identity_is_exact(c, 2, 5, 0, 7)
    assert lu == 5 == fr(c.runs[0][0]["min_base"]) < fr(c.runs[1][0]["min_base"])
    c = vc.CASES["tau_edge_8_8p5"]
    lu, lv = fr(c.ca[3, 0]) - fr(c.ca[0, 0]), fr(c.cb[2, 0]) - fr(c.cb[1, 0])
    assert (lu, lv) == (8, Fr(17, 2)) and c.ca[3, 1] == c.ca[0, 1] and c.cb[2, 1] == c.cb[1, 1]
    assert abs(lu - lv) == fr(c.runs[0][0]["tau_edge"]) > fr(c.runs[1][0]["tau_edge"])
    for name in ("tau_in_quarter", "tau_z_one"):
        c = vc.CASES[name]
        assert c.exact and _identity_is_exact(c, 1, 4, 1, 4) == 5
        dx, dy = fr(c.ca[6, 0]) - fr(c.cb[6, 0]), fr(c.ca[6, 1]) - fr(c.cb[6, 1])
        dz = abs(fr(c.ca[6, 2]) - fr(c.cb[6, 2]))
        d2 = dx * dx + dy * dy
        tin2 = [fr(f32(t["tau_in"]) * f32(t["tau_in"])) for t, _ in c.runs]
        tz = [fr(t["tau_z"]) for t, _ in c.runs]
        if name == "tau_in_quarter":
            assert d2 == Fr(1, 4) == tin2[0] > tin2[1] and dz == 0
        else:
            assert d2 == 0 and dz == 1 == tz[0] > tz[1]
    for name in ("tie_match_low_first", "tie_match_high_first"):
        c = vc.CASES[name]
        _identity_is_exact(c, 1, 4, 1, 4)
        d2 = [(fr(c.ca[6, 0]) - fr(c.cb[q, 0])) ** 2 + (fr(c.ca[6, 1]) - fr(c.cb[q, 1])) ** 2 for q in (3, 5)]
        assert d2[0] == d2[1] == Fr(1, 16) and c.cb[3, 1] != c.cb[5, 1]


def _three_sums(x, y):
    """x x + y y rounded per operation, and with either product fused into the sum (one rounding)."""
    x, y = f32(x), f32(y)
    return f32(f32(x * x) + f32(y * y)), round32(fr(x) ** 2 + fr(f32(y * y))), round32(fr(y) ** 2 + fr(f32(x * x)))


def test_rounding_literals_separate_the_fused_sum():
    for name, inside in (("round_inlier_separate_in", True), ("round_inlier_fused_in", False)):
        c = vc.CASES[name]
        _identity_is_exact(c, 1, 4, 1, 4)
        dx, dy = c.ca[6, 0] - c.cb[6, 0], c.ca[6, 1] - c.cb[6, 1]
        assert fr(dx) == fr(c.ca[6, 0]) - fr(c.cb[6, 0]) and fr(dy) == fr(c.ca[6, 1]) - fr(c.cb[6, 1])   # exact differences
        sep, f1, f2 = _three_sums(dx, dy)
        tin2 = f32(c.runs[0][0]["tau_in"]) * f32(c.runs[0][0]["tau_in"])
        assert f1 == f2 != sep
        assert (sep <= tin2 < f1) if inside else (f1 <= tin2 < sep), name
    for name, admitted in (("round_base_separate_longer", True), ("round_base_fused_longer", False)):
        c = vc.CASES[name]
        sep, f1, f2 = _three_sums(c.ca[5, 0] - c.ca[0, 0], c.ca[5, 1] - c.ca[0, 1])
        mb = f32(c.runs[0][0]["min_base"])
        assert f1 == f2 and np.sqrt(f1) != np.sqrt(sep)
        assert (np.sqrt(f1) < mb <= np.sqrt(sep)) if admitted else (np.sqrt(sep) < mb <= np.sqrt(f1)), name
    # subnormals: the distance and both thresholds are subnormal and non-zero
    c = vc.CASES["subnormal_inlier"]
    tiny = f32(1.1754943508222875e-38)
    dy = c.cb[2, 1] - c.ca[2, 1]
    assert 0 < dy * dy < tiny
    for t, _ in c.runs:
        assert 0 < f32(t["tau_in"]) * f32(t["tau_in"]) < tiny


def test_lattice_ties_span_batches_and_waves():
    c = vc.CASES["tie_lattice"]
    hyps, _ = vc.enumerate_hypotheses(c, vc.LATTICE_TOL)
    assert len(hyps) == ref("tie_lattice", 0)["hypotheses"] == 17568
    pts = {(int(x), int(y)) for x, y in c.ca[c.la >= 0, :2]}
    xy = {s: (int(c.ca[s, 0]), int(c.ca[s, 1])) for s in np.flatnonzero(c.la >= 0)}
    rots = [(1, 0), (0, 1), (-1, 0), (0, -1)]                  # (c, s)
    tied = []
    for n, (i, i2, j, j2) in enumerate(hyps):
        u = (xy[i2][0] - xy[i][0], xy[i2][1] - xy[i][1])
        v = (xy[j2][0] - xy[j][0], xy[j2][1] - xy[j][1])
        for cs, sn in rots:
            if (cs * u[0] - sn * u[1], sn * u[0] + cs * u[1]) == v:
                # the translation that maps a[i] on b[j]; a symmetry of the lattice maps all 25 nodes on nodes
                tx, ty = xy[j][0] - (cs * xy[i][0] - sn * xy[i][1]), xy[j][1] - (sn * xy[i][0] + cs * xy[i][1])
                if all((cs * x - sn * y + tx, sn * x + cs * y + ty) in pts for x, y in pts):
                    tied.append(n)
    assert len(tied) >= 300 and tied[0] == 0 and hyps[0] == (0, 1, 0, 1)
    keys = [hyps[n] for n in tied]
    assert min(keys) == hyps[0] and max(keys) != hyps[0]
    batches, waves = {n // 256 for n in tied}, {(n % 256) // 64 for n in tied}
    assert len(batches) >= 10 and waves == {0, 1, 2, 3}
    assert {n % 256 for n in tied[1:]} - {0}                   # ties in other lanes than the winner's


def test_cap_table_at_every_base_pair():
    c = vc.CASES["cap_12_nodes"]
    t = vc.tol()
    _, pairs = vc.enumerate_hypotheses(c, t)
    table = vc.cap_table(c, t)
    H = int(table[-1])
    assert len(pairs) == 66 and H > 100
    assert pairs[vc.CAP_ZERO_K][:2] == (5, 6) and pairs[vc.CAP_ZERO_K][3] == 0      # nodes 3 and 4 (slots 5 and 6)
    assert pairs[-1][3] >= 2 and set(vc.CAP_KS) >= {0, 65, vc.CAP_ZERO_K} and len(vc.CAP_KS) >= 10
    assert len({int(x) for x in table}) == 1 + sum(1 for p in pairs if p[3])        # every admissible pair adds to C
    for k in range(66):                                        # the whole sweep on the host
        for m in (int(table[k]), int(table[k]) + 1):
            if m < 1:
                continue
            r = geo_ref.verify_pair(c.ca, c.la, c.cb, c.lb, **vc.tol(max_hyp=m))
            assert (int(r["hypotheses"]), int(r["flags"])) == vc.cap_expect(table, m), (k, m)
    got = {t["max_hyp"]: e for t, e in c.runs}
    for k in vc.CAP_KS:
        ck = int(table[k])
        if ck >= 1:
            assert got[ck] == dict(hypotheses=ck, flags=vc.TRUNCATED)
        assert got[ck + 1]["hypotheses"] >= int(table[k + 1]) and got[ck + 1]["hypotheses"] > ck - (pairs[k][3] == 0)
    # the total is reached exactly by the last base pair: no base pair is started after it
    assert got[H] == got[H - 1] == dict(hypotheses=H, flags=0) and int(table[65]) < H - 1
    # ... unless one is: the short tail's last base pair is inadmissible and still counts as started
    c = vc.CASES["cap_12_nodes_short_tail"]
    _, pairs = vc.enumerate_hypotheses(c, t)
    table = vc.cap_table(c, t)
    H = int(table[-1])
    assert pairs[-1][3] == 0 and table[65] == H
    assert {t["max_hyp"]: e for t, e in c.runs} == {H - 1: dict(hypotheses=H, flags=vc.TRUNCATED),
                                                    H: dict(hypotheses=H, flags=vc.TRUNCATED),
                                                    H + 1: dict(hypotheses=H, flags=0)}


def test_structural_cases_reach_their_points():
    # compaction: where the real nodes of A sit
    la = vc.CASES["compact_last_wave_only"].la
    assert np.flatnonzero(la >= 0).tolist() == list(range(192, 256))
    assert np.flatnonzero(vc.CASES["compact_slots_0_and_255"].la >= 0).tolist() == [0, 255]
    for n_a in (63, 64, 65, 129):
        real = np.flatnonzero(vc.CASES["compact_holes_%d" % n_a].la >= 0)
        assert len(real) == n_a and len(set(real // 64)) == 4
        assert all(2 <= s % 64 < 62 for s in real)             # padding on both sides of every wave end
    # candidate chunks: 255 / 256 / 272 candidates in a base pair
    for (n1, n2), cand in (((15, 17), 255), ((16, 16), 256), ((16, 17), 272)):
        c = vc.CASES["chunk_ranges_%d_%d" % (n1, n2)]
        hyps, pairs = vc.enumerate_hypotheses(c, c.runs[0][0])
        assert sorted({p[2] for p in pairs}) == sorted({n1 * n1, n1 * n2, n2 * n2}) and cand in {p[2] for p in pairs}
        assert len(hyps) == ref(c.name, 0)["hypotheses"] > 0
    # ring and final flush
    want = {"flush_total_1": ([], 1), "flush_total_255": ([], 255), "flush_total_256": ([256], 0),
            "flush_total_1310": (None, 1310 % 256)}
    for name, (sizes, _) in vc.PRODUCT_CASES.items():
        c = vc.CASES[name]
        hyps, pairs = vc.enumerate_hypotheses(c, c.runs[0][0])
        assert all(p[2] == p[3] for p in pairs)                 # every candidate admissible
        assert len(hyps) == c.runs[0][1]["hypotheses"] == ref(name, 0)["hypotheses"]
        flushes, left = vc.ring_trace(pairs)
        if name in want:
            assert left == want[name][1] and (want[name][0] is None or flushes == want[name][0]), name
    _, pairs = vc.enumerate_hypotheses(vc.CASES["flush_total_256"], vc.CASES["flush_total_256"].runs[0][0])
    assert [p[2:] for p in pairs] == [(256, 256, (256,))]      # one base pair, exactly 256 admissible candidates
    _, pairs = vc.enumerate_hypotheses(vc.CASES["flush_total_1280"], vc.CASES["flush_total_1280"].runs[0][0])
    flushes, left = vc.ring_trace(pairs)
    assert [p[2] for p in pairs] == [200, 360, 720] and len(flushes) == 5 and left == 0     # empty final flush, ring wrapped
    assert 256 in flushes and max(flushes) > 256               # a flush at exactly 256 pending, and one above
    # the two enumerations agree wherever the cap is out of reach
    for c in vc.CASES.values():
        if c.group in ("cap",) or not c.finite:
            continue
        for n, (t, _) in enumerate(c.runs):
            assert len(vc.enumerate_hypotheses(c, t)[0]) == ref(c.name, n)["hypotheses"], (c.name, n)
    # tolerances 0: a graph against itself keeps every node
    assert ref("tolerances_all_zero", 0)["inliers"] == int((vc.CASES["tolerances_all_zero"].la >= 0).sum())


def test_nan_hypothesis_is_gone():
    """The finding: with min_base = 0 a base pair of two coincident nodes (lu = 0) was admissible against any B pair with
    0 < lv <= tau_edge; den = 0 made c = s = 0 / 0 and the NaN hypothesis won on its slot key.  Under lv_zero_ok (no
    den > 0 test at all) that record is still reproduced; the definition gives none."""
    r = ref("nan_hypothesis_alone", 0, "lv_zero_ok")
    assert r["flags"] == 0 and r["base"].tolist() == [0, 1, 2, 5] and r["hypotheses"] == 2 and np.isnan(r["coarse"]).all()
    assert np.isnan(r["refined"]).all() and np.isnan(r["rmse"])
    r = ref("nan_hypothesis_beside_finite", 0, "lv_zero_ok")
    assert r["flags"] == 0 and r["base"].tolist() == [0, 1, 2, 5] and np.isnan(r["coarse"]).all()
    r = ref("nan_hypothesis_beside_finite", 0)
    assert r["base"].tolist() == [4, 6, 6, 7] and r["coarse"].tolist() == [1.0, 0.0, -50.0, -50.0]
    c = vc.CASES["den_underflow"]
    lu = c.ca[1, 0] - c.ca[0, 0]
    assert lu > 0 and lu * lu == 0
