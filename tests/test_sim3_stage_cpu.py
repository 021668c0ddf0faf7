"""The references and probes of the stage tests of k_sim3_opt, without a device: sim3_stage_numpy against sim3opt_numpy, a census that
every probe of sim3_stage_cases reaches what it is there for, float64's distance d64 from long double per quantity with M d64 under the
caps, the float32 roundings of KannalaBrandt8, and which probes' counts are settled.  Run with -s for the figures."""
import numpy as np
import pytest

import sim3_stage_cases as sc
import sim3_stage_numpy as s3
import sim3opt_numpy as sn

# Trajectories that are cut (the number of budgets 1..k compared, see sc.trajectory_length).  KannalaBrandt8: after it float64 and long
# double have parted on the float32 staircase of theta and psi, and no bound of the form M d64 means anything.  reject-110 is a Pinhole
# case that starts 100 times as far off as Sim3Solver leaves an estimate, there for its rejected first plain trial (n1): its plain
# trajectory passes a cap at the ninth iteration, and it has no robust trajectory (sc.TRAJECTORIES)
CUT_TRAJECTORY = {("cam-kk-s1.0", "r"): 1, ("cam-kk-s1.0", "n"): 2, ("cam-pk-s1.0", "r"): 1, ("cam-pk-s1.0", "n"): 1,
                  ("reject-110", "n"): 8}
# probes on whose counts or flags float64 and long double differ: the GPU test allows the device a difference of one there
UNSETTLED = set()


def test_extended_precision_is_there():
    s3.require_extended()


@pytest.mark.parametrize("cname", ["seam-65", "cam-kk-s1.0", "cam-pk-s3.0", "seam-65-fs"])
def test_float64_run_restates_sim3opt_numpy(cname):
    """The same contract stated twice: in float64 the stage reference and tests/sim3opt_numpy.py agree on the linearisation to rounding
    and, for pinhole cameras, on the whole run."""
    pk = sc.case(cname)
    n = len(pk["info1"])
    chi, H, b, c12, c21 = sn.linearize(pk, pk["S12"], np.ones(n, bool), True)
    L = s3.first_linearization(pk, np.float64)
    assert abs(L.chi - chi) <= 1e-13 * chi
    assert np.abs(L.H - H).max() <= 1e-12 * np.abs(H).max() and np.abs(L.b - b).max() <= 1e-12 * np.abs(b).max()
    assert np.array_equal(L.c12, c12) and np.array_equal(L.c21, c21)
    if not (pk["kb8_1"] or pk["kb8_2"]):
        a, r = s3.run(pk, np.float64), sn.run(pk)
        assert tuple(a.iterations) == tuple(r.iterations) and a.round2 == r.round2
        assert np.array_equal(a.outlier1, r.outlier1) and np.array_equal(a.outlier, r.outlier) and a.n_in == r.n_in
        assert np.abs(a.S12 - r.S12).max() <= 1e-7


def test_budgets_of_zero_leave_the_input():
    r = s3.run(sc.probe("seam-65/e"))
    assert r.round2 and tuple(r.iterations) == (0, 0) and np.all(r.chi2_end == 0) and r.n_bad == 0
    assert np.array_equal(r.S12.astype(np.float64), sc.case("seam-65")["S12"])
    r = s3.run(sc.probe("seam-9/e"))
    assert not r.round2 and np.all(r.chi2_12 == 0)


# ------------------------------------------------------------------------------------------------------------- census
def _trace(name, rnd):
    return sc.refs(name).ld.trace[rnd]


@pytest.mark.parametrize("cname", [c for c in sc.LIN_CASES if not c.startswith(("seam-1", "seam-9")) or c == "seam-10"])
def test_census_both_sides_of_the_huber_threshold(cname):
    """At least a tenth of the edges of every robust linearisation probe is beyond the Huber threshold, and a tenth is within.  (These
    are also the cases of the robust one-iteration probes, but for `far`, where every edge is beyond it, and `near`, which has no noise to
    speak of and no edge beyond the threshold: near/r1 is a plain step under the robust label, there for the small-angle branch only.)"""
    L = sc.lin_refs(cname, True).ld
    over, total = int(L.over12.sum() + L.over21.sum()), 2 * len(L.c12)
    print(f"\n    {cname:18s} {over} of {total} edges beyond the Huber threshold", end="")
    assert 0.1 * total <= over <= 0.9 * total
    P = sc.lin_refs(cname, False).ld
    assert not P.over12.any() and not P.over21.any()


def test_census_rejections_stops_and_budgets():
    # a rejected first trial (plain), and rejected trials inside the robust trajectories
    rec = _trace(f"{sc.REJECT[0]}/n1", 1)[0]
    assert rec["qmax"] > 1 and rec["rho"][0] < 0 and rec["accepted"] and all(rec["ok"])
    robust_rejects = [(c, k) for c, m in sc.TRAJECTORIES if m == "r" for k, t in enumerate(_trace(f"{c}/r{sc.trajectory_length(c, 'r')}", 0))
                      if t["qmax"] > 1]
    print(f"\n    robust iterations with rejected trials: {robust_rejects}", end="")
    assert robust_rejects
    # the three-bad-iterations stop and a budget used up, in both rounds
    stops = {(rnd, t["stop"]) for name in ("seam-65/full", "far/full", "seam-65/b532", "limited/b532") for rnd in (0, 1)
             for t in _trace(name, rnd)}
    assert {(0, "nbad"), (1, "nbad"), (0, "budget"), (1, "budget")} <= stops, stops
    # n - n_bad == 10 and == 9
    a, b = sc.refs("twelve-2/full").ld, sc.refs("twelve-3/full").ld
    assert (12 - a.n_bad, a.round2) == (10, True) and (12 - b.n_bad, b.round2) == (9, False)
    # (5,3,2): the budget of round 2 for n_bad > 0 and for n_bad == 0, both used up
    a, b = sc.refs("seam-65/b532").ld, sc.refs("limited/b532").ld
    assert a.n_bad > 0 and a.budget2 == 3 and a.iterations[1] == 3
    assert b.n_bad == 0 and b.budget2 == 2 and b.iterations[1] == 2 and b.trace[1][0]["gain"] > 1e-2
    assert sc.refs("seam-65/full").ld.iterations[1] > 3 and sc.refs("limited/full").ld.iterations[1] > 2
    # a failed solve: ten of them, in both rounds
    z = sc.refs("zero-info/full").ld
    for rnd in (0, 1):
        assert len(z.trace[rnd]) == 1 and z.trace[rnd][0]["qmax"] == 10 and not any(z.trace[rnd][0]["ok"])
    assert tuple(z.iterations) == (1, 1) and z.round2 and z.n_in == 65 and np.all(z.chi2_end == 0)
    L = sc.lin_refs("far", True).ld                      # a start that far off: every edge is beyond the threshold
    assert L.over12.all() and L.over21.all()
    N = sc.lin_refs("near", True).ld
    assert not N.over12.any() and not N.over21.any()
    # the round-1 strict probe: the pair's long-double chi2 at the trial is 2e-8 or more inside both thresholds, in every float64 order too
    p, hi, lo = sc.strict_pair("converged", "round1")
    for which, flag in (("above", 0), ("below", 1)):
        r = sc.refs(f"converged/strict-round1-{which}")
        for run in [r.ld] + r.f64_orders:
            assert run.outlier1[p] == flag and run.iterations[0] == 1
        c = max(r.ld.chi2_round1[0][p], r.ld.chi2_round1[1][p])
        assert lo * (1 + 2e-8) < c < hi * (1 - 2e-8)
        print(f"\n    converged/strict-round1-{which}: chi2 {float(c):.10f} between {lo:.10f} and {hi:.10f}", end="")
    # the small-angle branch of the Sim3 exponential (theta < 1e-5) and far above it
    for name, lo, hi in (("near/r1", 0.0, 1e-5), ("near/n1", 0.0, 1e-5), ("far/r1", 1e-2, 1.0), ("far/n1", 1e-2, 1.0)):
        rnd = 0 if name.endswith("r1") else 1
        th = [float(np.sqrt((x[:3] ** 2).sum())) for x in _trace(name, rnd)[0]["x"]]
        print(f"\n    {name}: step rotation {th[-1]:.2e} rad", end="")
        assert all(lo < t < hi for t in th), (name, th)


# ------------------------------------------------------------------------------------------------------------- d64 and the caps
def test_float64_is_within_the_caps_on_every_probe():
    """M d64 <= cap for every compared quantity of every probe (KannalaBrandt8 trajectories are cut where it would not be), and the
    largest d64 per quantity."""
    worst, over = {}, []
    for name in sc.all_probes():
        for k, (d64, _) in sc.bounds(name).items():
            if sc.M * d64 > sc.CAPS[k]:
                over.append((name, k, d64))
            if d64 > worst.get(k, (0.0, ""))[0]:
                worst[k] = (d64, name)
    for c in sc.LIN_CASES:
        for robust in (True, False):
            for k, (d64, _) in sc.lin_bounds(c, robust).items():
                if sc.M * d64 > sc.LIN_CAPS[k]:
                    over.append((c, robust, k, d64))
                if d64 > worst.get(k, (0.0, ""))[0]:
                    worst[k] = (d64, f"{c}/{'lr' if robust else 'lp'}")
    print("\n    largest d64: " + "  ".join(f"{k} {v[0]:.1e} ({v[1]})" for k, v in worst.items()), end="")
    assert not over, over


def test_kb8_roundings_agree_between_float64_and_long_double():
    """The exclusion rule: a pair may be left out of a KannalaBrandt8 comparison only when its float32 roundings differ between the two
    references.  No committed case has such a pair, so the GPU tests leave nothing out."""
    for c in sc.LIN_CASES + sc.ERROR_CASES:
        pk = sc.case(c)
        if pk["kb8_1"] or pk["kb8_2"]:
            assert len(sc.rounding_mismatches(c)) == 0, c
            J12, J21 = s3.jacobians(s3.Problem(pk, np.longdouble), s3.Problem(pk, np.longdouble).S0)
            zeros = [float(np.mean(J[..., :6] == 0)) for J, kb in ((J12, pk["kb8_1"]), (J21, pk["kb8_2"])) if kb]
            print(f"\n    {c:18s} exactly zero entries of the KannalaBrandt8 Jacobians: " + " ".join(f"{z:.0%}" for z in zeros), end="")


def test_trajectory_lengths_and_settled_counts():
    got = {(c, m): sc.trajectory_length(c, m) for c, m in sc.TRAJECTORIES}
    print("\n    trajectory lengths: " + "  ".join(f"{c}/{m} {k}" for (c, m), k in got.items()), end="")
    for key, k in got.items():
        if key in CUT_TRAJECTORY:
            assert k == CUT_TRAJECTORY[key], (key, k)
        else:
            assert k == sc._budget_left(*key) and k >= 3, (key, k)
    unsettled = {name for name in sc.all_probes() if not sc.settled(name)}
    print(f"\n    unsettled probes: {sorted(unsettled)}", end="")
    assert unsettled == UNSETTLED
