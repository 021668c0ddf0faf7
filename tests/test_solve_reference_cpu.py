"""The reference of the solver tests (solve_reference.py) and the windows they run (solve_cases.py), vetted on the CPU.

For every window spec of test_gpu_solve.py, with (S, b_s) of the oracle's own linearisation: the long-double refinement converges,
the oracle's float64 no-pivot LDL^T (``ob.ldlt_solve``, the stand-in for SimplicialLDLT) meets no zero pivot, and its forward error
stays below 1e-6, so the yardstick the device is held to means something.  The figures are printed (pytest -s)."""
import numpy as np
import pytest

import solve_cases as sc
import solve_reference as sr


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


def test_reference_on_a_system_with_a_known_solution():
    sr.require_extended()
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.normal(size=(60, 60)))
    A = (Q * np.logspace(0, 8, 60)) @ Q.T          # SPD, condition number 1e8
    A = 0.5 * (A + A.T)
    x_true = rng.normal(size=60)
    b_ld = A.astype(sr.LD) @ x_true.astype(sr.LD)
    b = b_ld.astype(np.float64)
    S = np.triu(A) + np.tril(rng.normal(size=(60, 60)), -1)     # the strict lower triangle is scratch: never read
    x, info = sr.solve_refined(S, b)
    assert x.dtype == sr.LD and info["converged"] and np.array_equal(info["A"], A)
    assert all(b2 < a for a, b2 in zip(info["history"], info["history"][1:]))
    # b was rounded to float64: x solves the rounded system, 2^-53 |b| / sigma_min away from x_true at the most
    assert sr.forward_error(x, x_true) <= 60 * 2.0 ** -53 * np.abs(b).max() / 1.0 / np.abs(x_true).max()
    assert sr.backward_error(info, x) <= 2.0 ** -60
    x64 = np.linalg.solve(A, b)
    eta, eps = sr.errors(info, x, x64)
    assert 0 < eta <= 64 * sr.U53 and sr.U53 < eps < 1e-6           # a float64 solve: stable, and off by about kappa 2^-53
    assert sr.backward_error(info, x64 * (1 + 1e-6)) > 1e-8         # a wrong answer has a large backward error
    assert sr.forward_error(x64 * (1 + 1e-6), x) > 5e-7


def _vet(ob, w, lam, x_oracle=None):
    S, bs, xo = ob.lba_schur_step(w, lam)
    n = S.shape[0]
    x_ref, info = sr.solve_refined(S, bs)
    assert info["converged"], info["history"]
    if x_oracle is None:
        ok, x = ob.ldlt_solve(info["A"], bs)
        assert ok, "the oracle's LDL^T met a zero pivot"
        assert np.array_equal(x, xo[:n])          # lba_schur_step solves with the same routine
    else:
        x = xo[:n]
    eta, eps = sr.errors(info, x_ref, x)
    fill = np.count_nonzero(np.triu(S)) / (n * (n + 1) / 2)
    print(f"poses {w.n_free:4d} n {n:5d} edges {w.n_edges:6d} lambda {lam:g}: sweeps {len(info['history']) - 1} fill {fill:.2f} "
          f"oracle eta {eta:.2e} eps {eps:.2e}")
    assert eps < 1e-6 and eta <= 16 * sr.U53
    assert np.bincount(w.edge_pose[w.edge_pose < w.n_free], minlength=w.n_free).min() >= 6, "a pose with hardly any edge"
    return fill


@pytest.mark.parametrize("poses,style", sc.SMALL_SPECS)
def test_small_windows_suit_the_solver_tests(ob, poses, style):
    w = sc.window(poses, style)
    assert w.n_free == poses and 20 <= w.n_points / max(poses, 2) <= 60
    fills = [_vet(ob, w, lam) for lam in sc.LAMBDAS]
    if style == "long":
        assert min(fills) == 1.0                  # a dense S
    elif poses >= 6:
        assert max(fills) < 0.9                   # blocks above a ragged envelope


@pytest.mark.parametrize("poses,n_points", sc.SWITCH_LDS + sc.BACKSUB_GLOBAL + sc.SWITCH_BIG)
def test_switch_point_windows_suit_the_solver_tests(ob, poses, n_points):
    """(At the smaller lambda only, the worse conditioned system; the solution is lba_schur_step's own: the same routine.)"""
    _vet(ob, sc.switch_window(poses, n_points), min(sc.LAMBDAS), x_oracle="schur_step")


def test_zero_pivot_window_has_one_and_the_other_has_none(ob):
    w = sc.zero_pivot_window()
    S, bs, _ = ob.lba_schur_step(w, 1e-3)
    p = sc.ZERO_PIVOT_POSE
    blk = sr.symmetric(S)[6 * p:6 * p + 6]
    assert np.array_equal(blk[:, 6 * p:6 * p + 6], 1e-3 * np.eye(6)) and np.count_nonzero(blk) == 6 and not bs[6 * p:6 * p + 6].any()
    A0 = sr.symmetric(S) - 1e-3 * np.eye(S.shape[0])
    A0[6 * p:6 * p + 6, 6 * p:6 * p + 6] = 0.0   # (the other diagonal entries: lambda = 0 up to rounding, which cannot make them zero)
    ok, _ = ob.ldlt_solve(A0, bs)
    assert not ok
    # the window test_gpu_lba.py calls a zero-pivot window has none: every trial of the oracle is accepted at once
    w2 = sc.edgeless_landmark_window()
    r = ob.lba_solve(w2)
    assert r.iterations >= 5 and np.all(r.trials_trace[:r.iterations] == 1)
    S2, bs2, _ = ob.lba_schur_step(w2, 1e-3)
    assert np.diag(S2).min() > 1e3 and ob.ldlt_solve(sr.symmetric(S2), bs2)[0]
