"""Stage checks of k_sim3_opt and k_sim3_lin (csrc/sim3opt_device.hip) through their own inputs.  The kernel's three budgets are inputs
(osh_sim3_problem.iterations), so one stage at a time shows in the ordinary outputs:

    budgets (0,0,0), n >= 10            both edges' chi2 of every pair at the input S12, and the final classification
    osh_sim3_linearize, th2 / 1e30f     robust / plain H, b and chi2 at the input S12
    budgets (k,0,0)                     k robust iterations: iterations[0], chi2_end[0], outlier1, n_bad, and with 10 inliers S12 after round 1
    budgets (0,k,k)                     k plain iterations over every pair, S12, the final classification
    budgets (5,3,2)                     which round-2 budget was taken

The reference is tests/sim3_stage_numpy.py in long double (checked on the CPU by tests/test_sim3_stage_cpu.py); cases and probes are those
of tests/sim3_stage_cases.py.

Bound.  For every compared quantity d_dev = |device - long double| and d64 = |the same code in float64 - long double|, both relative to the
quantity; asserted: d_dev <= max(M d64, 8 ulp), and always a cap.
    pair_chi2   a pair's two chi2 where they were last computed at the exported S12, against long double AT THE DEVICE'S OWN S12, relative to
                max(chi2, 1e-3), worst pair; cap 1e-10
    trial_chi2  a pair's chi2 at an estimate that is not exported (the last trial of round 1), against the reference's run, relative to
                max(chi2, 1): its error goes with sqrt(chi2), see sim3_stage_cases; cap 1e-5
    chi2_end, S12 (rotation in rad, relative translation, relative scale) after iterations; H over s_i s_j and b over s_i sqrt(chi2),
                s_i = sqrt(max(H_ii, 1e-12 max diag)), entry by entry: cap 1e-5, the forward error of the 1e-9 central differences
    chi2 of osh_sim3_linearize: cap 1e-10
Counts and flags (iterations, round2, n_bad, n_in, outlier1, outlier) are equal where long double and float64 agree on them, which they do
on every probe here.

d64 is the largest over four fixed orders of the pairs (sim3_stage_cases.orders): after a few iterations the distance of one float64 run
from long double varies thirtyfold with the order of its sums, and one run alone understates the reference's own error (against a single
run the device reached a ratio of 25 on limited/b532, chi2_end, within the spread of the float64 runs themselves).

M = 16.  Worst d_dev / d64 per family, measured on an MI355X over the comparisons with d_dev above the 8-ulp floor; the tests print every
line with -s and the table at the end of the module:
    family          pair_chi2  trial_chi2  chi2_end   rot    trans  scale    H      b     chi2(lin)   worst probe
    errors             1.02        -          -        -       -      -      -      -       -         cam-kk-s1.0/e
    linearisation       -          -          -        -       -      -     1.49   3.13    1.00       norm-kk/lp (b)
    one iteration      2.04       1.00       1.03     2.44    2.07   2.40    -      -       -         norm-kk/r1
    trajectory         3.04       1.78       2.04     2.02    1.92   1.58    -      -       -         far/r6
    reject             0.52        -         1.00     1.00    1.00   1.00    -      -       -         reject-110/n1
    stops              0.63       1.08       0.60     1.89    1.86   1.05    -      -       -         seam-65/b532
    classification     1.00       1.36       1.24     0.71    0.76   0.23    -      -       -         twelve-3/full
    storage            0.83       0.87       3.29     1.38    1.04   2.49    -      -       -         seam-513-rotated/n3
Worst ratio 3.29, times 4 of headroom for a compiler release that orders the sums or contracts differently = 13.2, so M = 16.  M d64 stays
under the caps on every probe (test_sim3_stage_cpu.py); the largest d64 are 5.1e-12 (pair_chi2), 1.8e-5 (trial_chi2), 4.8e-7 (chi2_end),
9.9e-8 rad, 1.5e-7 (translation), 7.7e-8 (scale), 4.0e-7 (H), 1.2e-7 (b) and 6.6e-15 (chi2 of a linearisation).  KannalaBrandt8
trajectories are compared for 1 robust and 2 plain iterations (both cameras KannalaBrandt8) and 1 and 1 (Pinhole / KannalaBrandt8); after
that float64 and long double part on the float32 staircase of theta and psi.  The whole module runs in about four seconds.

What each test reaches in the kernel is said in its docstring.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import sim3_stage_cases as sc
import sim3_stage_numpy as s3
from orb_slam3_study_kr_amd import capi, lba

pytestmark = pytest.mark.gpu

FIELDS = ("S12", "outlier1", "outlier", "chi2_12", "chi2_21")
SCALARS = ("n_bad", "n_in", "round2", "iterations", "chi2_end")
_worst = {}          # family -> quantity -> (ratio, probe)
_worst_median = {}   # quantity -> (ratio against the median of the four float64 distances, probe)


@pytest.fixture(scope="module")
def solver(hip_lib):
    with lba.LbaSolver(0) as s:
        yield s
    print("\nworst d_dev / d64 per family (comparisons above the floor):")
    for fam, q in _worst.items():
        print(f"    {fam:16s} " + "  ".join(f"{k} {v[0]:.2f} ({v[1]})" for k, v in q.items()))
    print("worst d_dev against the MEDIAN of the four float64 distances: " + "  ".join(f"{k} {v[0]:.2f} ({v[1]})" for k, v in _worst_median.items()))


_device = {}


def device(solver, name):
    if name not in _device:
        _device[name] = solver.optimize_sim3([sc.probe(name)])[0]
    return _device[name]


def _judge(family, name, d_dev, bound, caps, median):
    line = []
    for k, d in d_dev.items():
        d64 = bound[k][0]
        ratio = d / d64 if d64 > 0 else (0.0 if d == 0 else float("inf"))
        line.append(f"{k} {d:.1e}|{d64:.1e} x{ratio:.2f}")
        if d > sc.FLOOR:
            if ratio > _worst.setdefault(family, {}).get(k, (0.0, ""))[0]:
                _worst[family][k] = (ratio, name)
            rm = d / median[k] if median[k] > 0 else float("inf")
            if rm > _worst_median.get(k, (0.0, ""))[0]:
                _worst_median[k] = (rm, name)
    print(f"\n    {name:30s} " + "  ".join(line), end="")
    for k, d in d_dev.items():
        assert d <= bound[k][1], (name, k, d, bound[k])
        assert d <= caps[k], (name, k, d)


def check(family, name, got, ref_name=None):
    """Every output of `got` against the references of probe `ref_name` (default: name)."""
    ref_name = ref_name or name
    r = sc.refs(ref_name).ld
    if sc.settled(ref_name):
        np.testing.assert_array_equal(got.iterations, r.iterations, err_msg=name)
        assert (got.round2, got.n_bad, got.n_in) == (r.round2, r.n_bad, r.n_in), name
        np.testing.assert_array_equal(got.outlier1, r.outlier1, err_msg=name)
        np.testing.assert_array_equal(got.outlier, r.outlier, err_msg=name)
    else:
        assert np.abs(np.asarray(got.iterations) - r.iterations).max() <= 1, name
    # the flags follow the device's own chi2 wherever that chi2 is still the one that was compared
    th2 = float(np.float32(sc.probe(ref_name)["th2"]))
    over = (got.chi2_12 > th2) | (got.chi2_21 > th2)
    np.testing.assert_array_equal(got.outlier.astype(bool), over, err_msg=name)
    assert got.n_bad == int(got.outlier1.sum()) and np.all(got.outlier1 <= got.outlier)
    if got.round2:
        assert got.n_in == len(over) - int(got.outlier.sum())
    else:
        assert got.n_in == 0 and np.array_equal(got.outlier, got.outlier1)
        np.testing.assert_array_equal(got.S12, sc.probe(ref_name)["S12"], err_msg=name)     # g2oS12 untouched, bit for bit
    if sc.probe(ref_name)["fix_scale"]:
        assert got.S12[7] == sc.probe(ref_name)["S12"][7]
    _judge(family, name, sc.distances(ref_name, got), sc.bounds(ref_name), sc.CAPS, sc.d64_median(ref_name))


def assert_same_bits(a, b, what):
    for fld in FIELDS:
        np.testing.assert_array_equal(getattr(a, fld), getattr(b, fld), err_msg=f"{what}: {fld}")
    assert all(getattr(a, f) == getattr(b, f) for f in SCALARS), what


# ------------------------------------------------------------------------------------------------- a. errors
@pytest.mark.parametrize("cname", sc.ERROR_CASES)
def test_errors_at_the_input(solver, cname):
    """Budgets (0,0,0): no iteration, every pair an inlier of round 1, and the final classification computes both edges of every pair at
    the input S12: obs1 - cam1(S12 X2c) and obs2 - cam2(S12^-1 X1c) for Pinhole and KannalaBrandt8 on either side, scales 0.5, 1 and 3 of
    S12, pairs whose obs2 are normalised coordinates, and 10 .. 1500 pairs around the seams of the 256-thread pair loop."""
    got = device(solver, f"{cname}/e")
    assert tuple(got.iterations) == (0, 0) and got.chi2_end == (0.0, 0.0) and got.round2 and got.n_bad == 0
    np.testing.assert_array_equal(got.S12, sc.case(cname)["S12"])
    check("errors", f"{cname}/e", got)
    norm = sc.case(cname)["normalised"]
    if norm.any():     # hundreds of pixels off through camera 2: that is the reference, and the device says so too
        assert np.all(got.chi2_21[norm] > 1e3) and np.all(got.outlier[norm] == 1)


def test_fewer_than_ten_pairs_without_iterations(solver):
    """n = 9 and n = 1 with budgets (0,0,0): 9 - 0 < 10 returns before anything is evaluated."""
    for cname in ("seam-9", "seam-1"):
        got = device(solver, f"{cname}/e")
        assert not got.round2 and got.n_in == 0 and got.n_bad == 0 and tuple(got.iterations) == (0, 0)
        np.testing.assert_array_equal(got.chi2_12, 0.0)
        np.testing.assert_array_equal(got.S12, sc.case(cname)["S12"])


# ------------------------------------------------------------------------------------------------- b. linearisation
@pytest.mark.parametrize("robust", [True, False], ids=["robust", "plain"])
@pytest.mark.parametrize("cname", sc.LIN_CASES)
def test_linearisation(solver, cname, robust):
    """H, b and chi2 of buildSystem at the input S12, with round 1's Huber kernels and (th2 = 1e30f) without: the 14 perturbed states and
    their inverses, both edges' central differences, rho' on H and on b, the upper-triangle sums and the four-wavefront reduction, for
    1 .. 1500 pairs.  Every entry of H is compared on the scale of its own row and column, so the scale and translation rows count as
    much as the rotation rows.  With fix_scale row and column 6 are exactly zero."""
    chi, H, b = solver.linearize_sim3(sc.lin_pack(cname, robust))
    ld = sc.lin_refs(cname, robust).ld
    np.testing.assert_array_equal(H, H.T)
    if sc.case(cname)["fix_scale"]:
        assert np.all(H[6] == 0.0) and np.all(H[:, 6] == 0.0) and b[6] == 0.0
        assert np.all(ld.H[6] == 0) and ld.b[6] == 0
    name = f"{cname}/{'lr' if robust else 'lp'}"
    _judge("linearisation", name, sc.lin_distances(H, b, chi, ld), sc.lin_bounds(cname, robust), sc.LIN_CAPS, sc.lin_d64_median(cname, robust))


# ------------------------------------------------------------------------------------------------- c. one iteration
@pytest.mark.parametrize("name", sc.ONE_ITERATION_PROBES)
def test_one_iteration(solver, name):
    """One robust (r1) or plain (n1) iteration: lambda's start, the 7x7 LDL^T, exp(x) S12 with x[6] = 0 under fix_scale, the trial's chi2
    and one verdict of the controller; `far` steps 0.14 rad, far above the 1e-5 small-angle branch of the Sim3 exponential, `near` steps
    2e-6 rad, below it."""
    got = device(solver, name)
    assert got.iterations[0 if name.endswith("r1") else 1] == 1
    check("one iteration", name, got)


# ------------------------------------------------------------------------------------------------- d. trajectories
@pytest.mark.parametrize("cname,mode", sc.TRAJECTORIES)
def test_trajectory(solver, cname, mode):
    """Budgets 1 .. K, K the first budget the reference does not use up: chi2_end, the iteration count and S12 after every iteration, so
    each lambda update, each relinearisation at the accepted trial and the stop rule are pinned one by one.  KannalaBrandt8 trajectories
    are cut where float64 and long double part ways (test_sim3_stage_cpu.py states the lengths)."""
    K = sc.trajectory_length(cname, mode)
    assert K >= 1
    for k in range(1, K + 1):
        check("trajectory", f"{cname}/{mode}{k}", device(solver, f"{cname}/{mode}{k}"))


# ------------------------------------------------------------------------------------------------- e. rejections, the failed solve
def test_rejected_first_trial(solver):
    """The rejected-trial branch (rho < 0: lambda *= ni, ni *= 2, the same H solved again, the estimate kept): S12 and chi2_end after an
    iteration of several trials tell which trial was accepted, because every trial has a lambda of its own."""
    name = f"{sc.REJECT[0]}/n1"
    rec = sc.refs(name).ld.trace[1][0]
    assert rec["qmax"] > 1 and rec["accepted"]
    check("reject", name, device(solver, name))


def test_failed_solves_and_the_trial_limit(solver):
    """info1 = info2 = 0: H = 0, lambda = 0, no pivot is positive, x = 0 and tempChi = DBL_MAX ten times; both rounds end after one
    iteration on qmax == kLmMaxTrials with S12 where it was, every chi2 0 and every pair an inlier."""
    got = device(solver, "zero-info/full")
    assert tuple(got.iterations) == (1, 1) and got.chi2_end == (0.0, 0.0)
    assert got.round2 and got.n_bad == 0 and got.n_in == 65 and not got.outlier.any()
    np.testing.assert_array_equal(got.S12, sc.case("zero-info")["S12"])
    np.testing.assert_array_equal(got.chi2_12, 0.0)
    np.testing.assert_array_equal(got.chi2_21, 0.0)
    check("stops", "zero-info/full", got)


# ------------------------------------------------------------------------------------------------- f. stops and budgets
@pytest.mark.parametrize("name", sc.STOP_PROBES)
def test_stops_and_budgets(solver, name):
    """The three-bad-iterations stop in both rounds (seam-65/full), a budget used up in both (far/full round 1, b532 round 2), and which
    round-2 budget (5,3,2) takes: 3 with round-1 outliers (seam-65), 2 without (limited); 9 pairs run round 1 only."""
    got = device(solver, name)
    r = sc.refs(name).ld
    if name.endswith("b532"):
        assert got.iterations[1] == r.budget2 == (3 if got.n_bad > 0 else 2)
    check("stops", name, got)


def test_refused_budgets_leave_the_context_usable(solver):
    """A negative budget or one above OSH_SIM3_MAX_ITERATIONS is OSH_ERR_INVALID before any device work, from either entry point; the
    limit itself is taken; the context then solves as before."""
    before = solver.optimize_sim3([sc.probe("seam-65/full")])[0]
    for bad in ((-1, 10, 5), (5, -1, 5), (5, 10, -3), (capi.OSH_SIM3_MAX_ITERATIONS + 1, 10, 5), (5, 10, 2 ** 31 - 1)):
        with pytest.raises(capi.OshError, match="iterations") as err:
            solver.optimize_sim3([sc.probe("seam-10/full"), sc.with_probe(sc.case("seam-65"), bad)])
        assert err.value.code == capi.OSH_ERR_INVALID
        with pytest.raises(capi.OshError, match="iterations") as err:
            solver.linearize_sim3(sc.with_probe(sc.case("seam-65"), bad))
        assert err.value.code == capi.OSH_ERR_INVALID
    top = capi.OSH_SIM3_MAX_ITERATIONS
    assert_same_bits(solver.optimize_sim3([sc.with_probe(sc.case("seam-65"), (top, top, top))])[0],
                     solver.optimize_sim3([sc.with_probe(sc.case("seam-65"), (50, 50, 50))])[0], "the limit")
    assert_same_bits(solver.optimize_sim3([sc.probe("seam-65/full")])[0], before, "after the refusals")


# ------------------------------------------------------------------------------------------------- g. classification
def test_strict_compare_in_the_final_classification(solver):
    """chi2 > th2 with the float th2 as a double: th2 the float32 just above the long-double chi2 of a pair at the input S12 keeps it, the
    float32 just below rejects it.  That is 3e-8 relative, against a device chi2 that is 1e-13 from the reference at a given S12."""
    p, hi, lo = sc.strict_pair("seam-65", "final")
    above, below = device(solver, "seam-65/strict-final-above"), device(solver, "seam-65/strict-final-below")
    assert above.outlier[p] == 0 and below.outlier[p] == 1 and below.n_in == above.n_in - 1
    check("classification", "seam-65/strict-final-above", above)
    check("classification", "seam-65/strict-final-below", below)


def test_strict_compare_in_round_one(solver):
    """The same two thresholds in the round-1 classification.  After an ordinary step float64 itself is 1e-7 from long double in a pair's
    chi2, more than the 4.8e-8 to either threshold, so the case `converged` starts at the reference's converged robust estimate with one
    pair's chi2 halfway between the float32 10 and the float32 below it: one robust iteration (budgets (1,0,0)) moves that chi2 by
    1e-11, its trial is what round 1 classifies, and the verdict is fixed: inlier with th2 = 10, outlier with the float32 below."""
    p, hi, lo = sc.strict_pair("converged", "round1")
    above, below = device(solver, "converged/strict-round1-above"), device(solver, "converged/strict-round1-below")
    for name, ld in (("above", sc.refs("converged/strict-round1-above").ld), ("below", sc.refs("converged/strict-round1-below").ld)):
        c = max(ld.chi2_round1[0][p], ld.chi2_round1[1][p])
        assert lo * (1 + 2e-8) < c < hi * (1 - 2e-8), (name, c)
    assert above.iterations[0] == below.iterations[0] == 1
    assert above.outlier1[p] == 0 and below.outlier1[p] == 1 and below.n_bad == above.n_bad + 1
    check("classification", "converged/strict-round1-above", above)
    check("classification", "converged/strict-round1-below", below)


@pytest.mark.parametrize("name,left,round2", [("twelve-2/full", 10, True), ("twelve-3/full", 9, False)])
def test_ten_inliers_or_nine(solver, name, left, round2):
    """12 pairs with 2 and with 3 gross outliers: 10 inliers run round 2, 9 return with S12 as it came, bit for bit (check() asserts it),
    and with the round-1 outliers as the only ones."""
    got = device(solver, name)
    assert 12 - got.n_bad == left and got.round2 == round2
    check("classification", name, got)


def test_round_one_outliers_keep_their_round_one_chi2(solver):
    """seam-65/full: the chi2 of a round-1 outlier is the one round 1 classified it with (round 2 and the final classification skip it)."""
    got, r = device(solver, "seam-65/full"), sc.refs("seam-65/full").ld
    out = got.outlier1.astype(bool)
    assert out.any() and np.array_equal(out, r.outlier1.astype(bool))
    c12, c21 = r.chi2_round1
    assert np.abs(got.chi2_12[out] / c12[out].astype(np.float64) - 1).max() < sc.CAP_DIFF
    assert np.abs(got.chi2_21[out] / c21[out].astype(np.float64) - 1).max() < sc.CAP_DIFF
    final12, _ = s3.pair_chi2_at(sc.probe("seam-65/full"), got.S12)
    assert np.abs(final12[out].astype(np.float64) / got.chi2_12[out] - 1).max() > 1e-3     # and not the chi2 at the final estimate


# ------------------------------------------------------------------------------------------------- h. storage
@pytest.mark.parametrize("name", ["seam-513/full", "big-1500/full"])
def test_a_problem_at_any_place_of_a_batch(solver, name):
    """A problem alone, and first and last of a batch of 16 that holds both camera models (k_sim3_opt<true> then, and pair offsets up
    to 1500 + ...), gives the same bits: the reductions have a fixed order and every problem reads its own slice."""
    alone = device(solver, name)
    check("storage", name, alone)
    fill = [sc.probe(f"{c}/full") for c in ("cam-kk-s1.0", "seam-257", "cam-pk-s1.0", "seam-9", "seam-65", "cam-kp-s1.0", "seam-1", "far")] * 2
    for pos in (0, 15):
        batch = fill[:pos] + [sc.probe(name)] + fill[pos:15]
        assert len(batch) == 16
        assert_same_bits(solver.optimize_sim3(batch)[pos], alone, f"{name} at {pos}")


@pytest.mark.parametrize("p", ["r3", "n3", "full"])
def test_pairs_rotated_by_100(solver, p):
    """seam-513 with its first 100 pairs last: every pair sits on another thread and in another pass of the pair loop.  Same problem,
    other summation order: within the bound of the same reference."""
    got = device(solver, f"seam-513-rotated/{p}")
    rot = sc.rotation_100(513)                       # rotated pair i is pair rot[i] of seam-513

    def back(a):
        o = np.empty_like(a)
        o[rot] = a
        return o

    view = SimpleNamespace(S12=got.S12, iterations=got.iterations, chi2_end=got.chi2_end, n_bad=got.n_bad, n_in=got.n_in,
                           round2=got.round2, **{f: back(getattr(got, f)) for f in ("outlier1", "outlier", "chi2_12", "chi2_21")})
    check("storage", f"seam-513-rotated/{p}", view, ref_name=f"seam-513/{p}")
    check("storage", f"seam-513/{p}", device(solver, f"seam-513/{p}"))
