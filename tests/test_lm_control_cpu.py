"""The Levenberg-Marquardt controller every solver shares (csrc/g2o_lm.h) on the CPU: ``osh_lm_control_check`` plays it over a
script of trials {tempChi, computeScale sum, solve_ok}; the rule of g2o's optimization_algorithm_levenberg.cpp:99-169 is
restated here in a few lines and the two are compared on scripts that reach every branch.

Decisions, ni, nBad and the trial counts are compared exactly.  lambda is compared at relative 1e-14: each side calls the C
library's pow, whose results can differ by one ulp; the factor max(1/3, alpha) amplifies an absolute error in the cube by at
most 3, i.e. about 3.3e-16 per accepted trial, and no script has more than 12 accepted trials (4e-15 < 1e-14)."""
import math
import sys

import numpy as np
import pytest

from orb_slam3_study_kr_amd import capi

DBL_MAX = sys.float_info.max
MAX_TRIALS = 10


def play_native(chi, lam, script):
    lib = capi.load_library()
    n = len(script)
    s = np.ascontiguousarray(np.asarray(script, dtype=np.float64).reshape(n, 3))
    acc, go, nbad, tr = (np.full(n, -1, dtype=np.int32) for _ in range(4))
    rho, lm, ni = (np.full(n, np.nan) for _ in range(3))
    played = np.zeros(2, dtype=np.int32)
    i32, f64 = capi.c_int32_p, capi.c_double_p
    rc = lib.osh_lm_control_check(chi, lam, n, capi.ptr(s, f64), capi.ptr(acc, i32), capi.ptr(rho, f64), capi.ptr(lm, f64), capi.ptr(ni, f64),
                                  capi.ptr(go, i32), capi.ptr(nbad, i32), capi.ptr(tr, i32), capi.ptr(played, i32))
    assert rc == 0, lib.osh_last_error().decode()
    nt, nit = int(played[0]), int(played[1])
    trials = [(bool(acc[k]), float(rho[k]), float(lm[k]), float(ni[k])) for k in range(nt)]
    iters = [(bool(go[k]), int(nbad[k]), int(tr[k])) for k in range(nit)]
    return trials, iters


def play_python(chi, lam, script):
    """g2o's solve() per iteration inside optimize(): the same outputs as play_native."""
    trials, iters = [], []
    ni, n_bad, k, ok = 2.0, 0, 0, True
    while ok and k < len(script):
        ini, rho, qmax = chi, 0.0, 0
        while True:
            temp, scale, solve_ok = script[k]
            if not solve_ok:
                temp = DBL_MAX
            with np.errstate(all="ignore"):
                rho = np.float64(chi) - np.float64(temp)                 # numpy: inf / nan instead of exceptions
                rho = rho / np.float64(scale + 1e-3)
            good = bool(rho > 0 and math.isfinite(temp))
            if good:
                cube = float(2 * rho - 1) ** 3 if math.isfinite(rho) else math.inf
                lam *= max(1. / 3., min(1. - cube, 2. / 3.))
                ni, chi = 2.0, temp
            else:
                lam *= ni
                ni *= 2
            trials.append((good, float(rho), lam, ni))
            qmax += 1
            k += 1
            if not (rho < 0 and qmax < MAX_TRIALS and k < len(script)):
                break
        if rho < 0 and qmax < MAX_TRIALS:
            break                                                        # the script ended inside an iteration
        if qmax == MAX_TRIALS or rho == 0:
            ok = False
        else:
            n_bad = n_bad + 1 if (ini - chi) * 1e3 < ini else 0
            ok = n_bad < 3
        iters.append((ok, n_bad, qmax))
    return trials, iters


def good(chi, rho, scale=1.0):
    """A trial accepted from `chi` with gain ratio `rho` (up to rounding)."""
    return (chi - rho * (scale + 1e-3), scale, 1)


def chain(chi, rhos, scale=1.0):
    out = []
    for r in rhos:
        out.append(good(chi, r, scale))
        chi = out[-1][0]
    return out


SCRIPTS = {
    # alpha = 1 - (2 rho - 1)^3 below 1/3 (rho near 1 or large), inside [1/3, 2/3] (rho about 0.9), above 2/3 (rho about 0.5 or less)
    "alpha_below_clamp": (100.0, 1e-3, chain(100.0, [0.99, 0.999, 5.0])),
    "alpha_inside_clamp": (100.0, 1e-3, chain(100.0, [0.9, 0.91, 0.92])),   # (2 rho - 1)^3 = 0.512 .. 0.593: alpha in [1/3, 2/3]
    "alpha_above_clamp": (100.0, 1e-3, chain(100.0, [0.5, 0.1, 0.6])),
    "reject_then_accept": (100.0, 1e-3, [(120.0, 2.0, 1), (101.0, 1.0, 1), (60.0, 50.0, 1), (30.0, 40.0, 1)]),
    "rho_exactly_zero": (100.0, 1e-3, [(80.0, 30.0, 1), (80.0, 5.0, 1), (10.0, 1.0, 1)]),
    "non_finite_tempchi": (100.0, 1e-3, [(math.inf, 1.0, 1), (math.nan, 1.0, 1), (-math.inf, 1.0, 1), (50.0, 60.0, 1), (20.0, 40.0, 1)]),
    "failed_solve_dbl_max": (100.0, 1e-3, [(50.0, 60.0, 0), (DBL_MAX, 1.0, 1), (50.0, 60.0, 1), (25.0, 30.0, 1)]),
    "negative_scale_sum": (100.0, 1e-3, [(120.0, -5.0, 1), (90.0, -5.0, 1), (80.0, 12.0, 1)]),
    "ten_rejected_trials": (100.0, 1e-3, [(100.0 + k, 1.0, 1) for k in range(1, 11)] + [(1.0, 1.0, 1)]),
    "nine_rejected_then_accept": (100.0, 1e-3, [(100.0 + k, 1.0, 1) for k in range(1, 10)] + [(50.0, 60.0, 1), (20.0, 40.0, 1)]),
    "three_small_gain_iterations": (100.0, 1e-3, [(99.95, 0.1, 1), (99.91, 0.1, 1), (99.90, 0.1, 1), (1.0, 1.0, 1)]),
    "two_small_gains_then_a_good_one": (100.0, 1e-3, [(99.95, 0.1, 1), (99.91, 0.1, 1), (50.0, 60.0, 1), (49.99, 0.1, 1), (49.98, 0.1, 1),
                                                      (49.97, 0.1, 1), (1.0, 1.0, 1)]),
    "twelve_accepted_trials": (1e4, 7.5, chain(1e4, [0.3, 0.7, 0.55, 0.9, 0.2, 0.65, 0.45, 0.8, 0.35, 0.6, 0.5, 0.75], 100.0)),
    "script_ends_inside_an_iteration": (100.0, 1e-3, [(50.0, 60.0, 1), (70.0, 1.0, 1), (71.0, 1.0, 1)]),
}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_controller_matches_the_restated_rule(name):
    chi, lam, script = SCRIPTS[name]
    got_t, got_i = play_native(chi, lam, script)
    exp_t, exp_i = play_python(chi, lam, script)
    assert got_i == exp_i                                                # go-on decisions, nBad, trials per iteration
    assert len(got_t) == len(exp_t)
    for k, (g, e) in enumerate(zip(got_t, exp_t)):
        assert g[0] == e[0], (k, g, e)                                   # accepted
        assert g[1] == e[1] or (math.isnan(g[1]) and math.isnan(e[1])), (k, g, e)   # rho: a subtraction, an addition, a division
        assert g[3] == e[3], (k, g, e)                                   # ni: powers of two
        assert abs(g[2] - e[2]) <= 1e-14 * abs(e[2]), (k, g, e)          # lambda


def test_the_scripts_reach_every_branch():
    """What each script is there for, checked on the restated rule (so a script that drifts off its branch is noticed)."""
    played = {n: play_python(*SCRIPTS[n]) for n in SCRIPTS}
    factor = lambda n: [t[2] for t in played[n][0]]
    f = factor("alpha_below_clamp")
    assert f[0] / 1e-3 == pytest.approx(1. / 3.) and f[1] / f[0] == pytest.approx(1. / 3.) and f[2] / f[1] == pytest.approx(1. / 3.)
    f = factor("alpha_inside_clamp")
    assert all(1. / 3. < b / a < 2. / 3. for a, b in zip([1e-3] + f[:-1], f))
    f = factor("alpha_above_clamp")
    assert all(b / a == pytest.approx(2. / 3.) for a, b in zip([1e-3] + f[:-1], f))
    t, i = played["reject_then_accept"]
    assert [x[0] for x in t] == [False, False, True, True] and t[1][3] == 8.0 and i[0] == (True, 0, 3)
    t, i = played["rho_exactly_zero"]
    assert t[1][1] == 0.0 and not t[1][0] and i == [(True, 0, 1), (False, 0, 1)]
    t, i = played["non_finite_tempchi"]
    assert [x[0] for x in t] == [False, False, False, True, True] and math.isnan(t[1][1]) and t[2][1] == math.inf
    assert i[:2] == [(True, 1, 2), (True, 2, 1)]   # a NaN or +inf gain ratio ends the trial loop (rho < 0 is false) with nothing accepted
    t, i = played["failed_solve_dbl_max"]
    assert [x[0] for x in t] == [False, False, True, True]
    t, i = played["negative_scale_sum"]
    assert [x[0] for x in t] == [True, False, True] and t[0][1] > 0 and t[1][1] < 0
    t, i = played["ten_rejected_trials"]
    assert len(t) == 10 and i == [(False, 0, 10)] and t[-1][3] == 2.0 ** 11
    t, i = played["nine_rejected_then_accept"]
    assert t[9][0] and i == [(False, 0, 10)]                             # qmax == 10 stops even after an accepted tenth trial
    assert played["three_small_gain_iterations"][1] == [(True, 1, 1), (True, 2, 1), (False, 3, 1)]
    assert [x[1] for x in played["two_small_gains_then_a_good_one"][1]] == [1, 2, 0, 1, 2, 3]
    assert sum(x[0] for x in played["twelve_accepted_trials"][0]) == 12
    t, i = played["script_ends_inside_an_iteration"]
    assert len(t) == 3 and len(i) == 1
