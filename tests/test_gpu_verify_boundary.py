"""sgpr_verify_pairs on the MI355X ON its rules: every case of tests/verify_cases.py through engine.verify_pairs, every
record against tests/geo_ref.py BIT FOR BIT, plus the fields each case states.  tests/test_verify_boundary_host.py
proves (no GPU) that each case sits on the rule it is named for; a kernel with `<` for `<=`, a contracted sum, flushed
subnormals, a tie to the wrong side or a cap tested elsewhere computes what the matching altered reference computes, and
that differs on the cases listed in verify_cases.MUTANT_CASES.

Cases that share N and the tolerances go through one call; the cap sweep is one call per max_hyp."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_ref  # noqa: E402
import verify_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(name, n_run):
    """The reference record of one run of a case: computed once, shared by the tests, never modified."""
    if (name, n_run) not in _REF:
        c = vc.CASES[name]
        r = geo_ref.verify_pair(c.ca, c.la, c.cb, c.lb, **c.runs[n_run][0])
        r.setflags(write=False)
        _REF[(name, n_run)] = r
    return _REF[(name, n_run)]


def gpu_records(ca, la, cb, lb, ia, ib, **tol):
    from sg_pr_amd import engine
    tol = dict(tol)
    tol["tau_inlier"] = tol.pop("tau_in")
    out = engine.verify_pairs(np.asarray(ca, np.float32), np.asarray(la, np.int32), np.asarray(cb, np.float32),
                              np.asarray(lb, np.int32), np.asarray(ia, np.int32), np.asarray(ib, np.int32), **tol)
    torch.cuda.synchronize()
    return out["record"].cpu().numpy().view(engine.VERIFY_RESULT).reshape(-1)


def run_cases(names):
    """Every run of the named cases: batched by (N, tolerances), compared bit for bit and with the case's statements."""
    batches = collections.OrderedDict()
    for name in names:
        c = vc.CASES[name]
        for n, (t, _) in enumerate(c.runs):
            batches.setdefault((c.n,) + tuple(sorted(t.items())), []).append((name, n))
    got_all = {}
    for key, members in batches.items():
        t = dict(key[1:])
        cs = [vc.CASES[name] for name, _ in members]
        idx = np.arange(len(cs))
        got = gpu_records(np.stack([c.ca for c in cs]), np.stack([c.la for c in cs]), np.stack([c.cb for c in cs]),
                          np.stack([c.lb for c in cs]), idx, idx, **t)
        for (name, n), g in zip(members, got):
            want = _ref(name, n)
            bad = geo_ref.equal_records(np.array([g]), np.array([want]))
            if bad:
                raise AssertionError("%s run %d %s: fields %s differ\n gpu %s\n ref %s\nthe rules and their cases:\n%s" % (
                    name, n, t, bad, g, want, vc.mutant_table()))
            vc.check_expect(name, n, g, vc.CASES[name].runs[n][1])
            if vc.CASES[name].finite and g["flags"] == 0:      # "evaluated, no flag" never carries a NaN closure edge
                assert np.isfinite(g["coarse"]).all() and np.isfinite(g["refined"]).all(), (name, n, g)
            got_all[(name, n)] = g
    return got_all


def test_comparisons_at_and_one_float_from_their_thresholds():
    """lu >= min_base, |lu - lv| <= tau_edge, d2 <= tau_in^2, |dz| <= tau_z with equality and one float32 away; den > 0."""
    got = run_cases(vc.GROUPS["comparisons"])
    for name in ("min_base_3_4_5", "tau_edge_8_8p5", "tau_in_quarter", "tau_z_one"):
        assert geo_ref.equal_records(np.array([got[(name, 0)]]), np.array([got[(name, 1)]])) != [], name


def test_sums_are_rounded_per_operation_and_subnormals_kept():
    """dx dx + dy dy and ux ux + uy uy one ulp from their thresholds where a fused multiply-add lands on the other side;
    a subnormal distance against a subnormal tau_in^2."""
    got = run_cases(vc.GROUPS["rounding"])
    assert got[("subnormal_inlier", 0)]["inliers"] == 3 and got[("subnormal_inlier", 1)]["inliers"] == 2


def test_ties_go_to_the_lowest_key_and_the_lowest_slot():
    """25-inlier ties in every evaluation batch and wave of a lattice: the identity on the lowest base pair wins; two
    nodes of B equally far from a projected node: q(p) is the lower slot."""
    got = run_cases(vc.GROUPS["ties"])
    assert got[("tie_match_low_first", 0)]["refined"][3] < 0 < got[("tie_match_high_first", 0)]["refined"][3]


def test_cap_is_tested_before_every_base_pair():
    """max_hyp = C_k stops before base pair k (TRUNCATED, hypotheses = C_k), C_k + 1 goes on through it; the total reached
    by the last base pair is no truncation, reached before an inadmissible last base pair it is."""
    got = run_cases(vc.GROUPS["cap"])
    assert len(got) >= 24


def test_refinement_fallbacks():
    """No inlier (NaN rmse), one inlier, two inliers whose nodes of A coincide (nrm == 0): the coarse transform widened."""
    run_cases(vc.GROUPS["fallbacks"])


def test_no_nan_hypothesis():
    """lu = 0 at min_base = 0, and lu lv underflowing to 0, are inadmissible: NO_HYPOTHESIS, or the finite hypothesis."""
    got = run_cases(vc.GROUPS["fix"])
    assert got[("nan_hypothesis_beside_finite", 0)]["coarse"].tolist() == [1.0, 0.0, -50.0, -50.0]


def test_compaction_chunks_ring_and_tolerance_ends():
    """A's compaction with whole waves empty and holes over the wave ends, 255 / 256 / 272 candidates per base pair, 1 / 255
    / 256 / 1280 / 1310 admissible hypotheses (no flush, exactly one, a wrapped ring with an empty final flush, a partial
    one), tolerances 0 and +inf, coordinates whose squares overflow."""
    got = run_cases(vc.GROUPS["structure"])
    r = got[("overflowing_coordinates", 0)]                    # pinned, not promised (include/sgpr.h)
    assert r["flags"] == 0 and r["coarse"].tolist() == [0.0, 0.0, 0.5, 0.5] and np.signbit(r["coarse"][:2]).all()


def test_every_case_is_run():
    assert sorted(sum(vc.GROUPS.values(), [])) == sorted(vc.CASES)
    assert set(vc.GROUPS) == {"comparisons", "rounding", "ties", "cap", "fallbacks", "fix", "structure"}
