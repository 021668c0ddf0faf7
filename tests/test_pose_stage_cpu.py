"""The reference of the stage tests of k_pose_opt (tests/pose_stage_numpy.py) and their cases (tests/pose_stage_cases.py), checked without
a GPU: the analytic Jacobians against central differences, the float64 run against oracle/pose_oracle.c on every probe, the properties
the cases are there for (rejected trials, the stop rules, a round without active edges) and that no cap is what lets a probe pass."""
import numpy as np
import pytest

import pose_stage_cases as pc
import pose_stage_numpy as ps


def test_long_double_is_extended():
    ps.require_extended()


@pytest.mark.parametrize("fname,kinds", [("seam-257", (ps.MONO, ps.STEREO)), ("mono", (ps.MONO,)), ("kb8", (ps.MONO,)), ("rig", (ps.MONO, ps.BODY))])
def test_analytic_jacobians_against_central_differences(fname, kinds):
    """d _error / d x of exp(x) T at x = 0, in long double.  The reference library's Jacobians are those of the unrounded projection, so
    the differenced residual leaves the float32 roundings out: `smooth` for theta and psi of KannalaBrandt8, and u - bf / z in place of
    the float32 1/z and bf product for the third row of the stereo edge."""
    ps.require_extended()
    L = np.longdouble
    P = ps.Problem(pc.frame(fname), L)
    qt = np.concatenate([ps.normalize_rotation(P.qt0[:4]), P.qt0[4:]])
    J = ps.jacobians(P, qt)

    def smooth_residual(q):
        r, Xc = ps.residuals(P, q, smooth=True)
        i = P.i_st
        if i.size:
            u = P.cam[0] * Xc[i, 0] / Xc[i, 2] + P.cam[2]
            v = P.cam[1] * Xc[i, 1] / Xc[i, 2] + P.cam[3]
            r[i, 0], r[i, 1], r[i, 2] = P.obs[i, 0] - u, P.obs[i, 1] - v, P.obs[i, 2] - (u - P.cam[4] / Xc[i, 2])
        return r

    h = L(1e-6)
    for k in range(6):
        x = np.zeros(6, dtype=L)
        x[k] = h
        fd = (smooth_residual(ps.pose_oplus(x, qt)) - smooth_residual(ps.pose_oplus(-x, qt))) / (2 * h)
        scale = np.abs(J).max(axis=(1, 2))
        err = np.abs(fd - J[:, :, k]).max(axis=1) / scale
        assert err.max() < 1e-9, (fname, k, float(err.max()))        # truncation h^2 = 1e-12 times the third derivative
    for kind in kinds:
        assert (P.kind == kind).sum() > 20


ALL = pc.all_probes()


@pytest.mark.parametrize("name", ALL)
def test_float64_reference_against_the_oracle(name):
    """Two independent restatements in the same arithmetic: same iteration counts, and the oracle, the float64 run and the long-double
    run within the caps of each other.  M d64 <= cap: the bound of the GPU test is never the cap."""
    r = pc.refs(name)
    assert r.f64.rounds == r.oracle.rounds == r.ld.rounds
    if pc.settled(name):
        np.testing.assert_array_equal(r.f64.iterations, r.oracle.iterations)
    else:
        assert np.abs(r.f64.iterations - r.oracle.iterations).max() <= 1
    np.testing.assert_array_equal(r.f64.outlier, r.oracle.outlier)
    np.testing.assert_array_equal(r.ld.outlier, r.oracle.outlier)
    assert r.f64.n_bad == r.oracle.n_bad == r.ld.n_bad
    for who, d in (("f64", pc.distances(r.f64, r.ld)), ("oracle-f64", pc.distances(r.oracle, r.f64))):
        for k, v in d.items():
            assert v <= pc.CAPS[k], (name, who, k, v)
    for k, (d64, bound) in pc.bounds(name).items():
        assert pc.M * d64 <= pc.CAPS[k], (name, k, d64)
        assert bound <= pc.CAPS[k]


def test_most_stop_decisions_are_settled():
    names = pc.trajectory_probes()
    share = sum(pc.settled(n) for n in names) / len(names)
    assert share >= 0.8, share


@pytest.mark.parametrize("fname", list(pc.REJECT))
def test_far_frames_reject_trials(fname):
    """The long-double trace takes more than one trial in the stated iteration; at least one case takes three or more, where lambda *= ni
    and lambda *= 2 part."""
    for rnd, it in pc.REJECT[fname][3].items():
        mode = "r" if rnd == 0 else "n"
        for run in (pc.refs(f"{fname}/{mode}10"), pc.refs(f"{fname}/{mode}{it + 1}")):
            rec = run.ld.trace[rnd][it]
            assert rec["qmax"] > 1 and rec["qmax"] == run.f64.trace[rnd][it]["qmax"], (fname, rnd, it, rec["qmax"])
            assert all(rho < 0 for rho in rec["rho"][:-1]) and rec["rho"][-1] > 0
    worst = max(pc.refs(f"{fn}/{'r' if rnd == 0 else 'n'}10").ld.trace[rnd][it]["qmax"] for fn in pc.REJECT for rnd, it in pc.REJECT[fn][3].items())
    assert worst >= 3


def _stops(name):
    return [rec["stop"] for rnd in pc.refs(name).ld.trace for rec in rnd]


def test_every_exit_of_the_iteration_loop_is_reached_by_a_probe():
    assert _stops("exact/full") == ["rho0"] * 4                                  # rho == 0
    assert "rho0" in _stops("rig/readmit")
    assert "nbad" in _stops("reject-88/n10") and "nbad" in _stops("seam-257/r10")  # three iterations below 0.1 % gain
    assert "budget" in _stops("reject-89/r10")
    assert _stops("zero-info/full") == ["trials"] * 4                            # qmax == 10 through failed solves
    assert "trials" in _stops("seam-257/readmit")                                # qmax == 10 through rejected trials of good solves
    for name in ("seam-257/allout", "rig/allout"):                               # a round without active edges
        r = pc.refs(name).ld
        assert r.no_active == [False, True, False, False] and r.iterations[1] == 0 and r.chi2_final[1] == 0
        assert r.iterations[2] > 0 and r.iterations[3] > 0


def test_zero_information_fails_every_solve():
    r = pc.refs("zero-info/full")
    for run in (r.ld, r.f64, r.oracle):
        np.testing.assert_array_equal(run.iterations, [1, 1, 1, 1])
        np.testing.assert_array_equal(np.asarray(run.chi2_final, dtype=np.float64), 0.0)
    for rnd in r.ld.trace:
        assert rnd[0]["qmax"] == ps.MAX_TRIALS and rnd[0]["lam0"] == 0
    f = pc.frame("zero-info")
    q = f.pose_qt[:4] / np.linalg.norm(f.pose_qt[:4]) * (1 if f.pose_qt[3] >= 0 else -1)
    np.testing.assert_allclose(np.asarray(r.ld.pose_qt, dtype=np.float64), np.concatenate([q, f.pose_qt[4:]]), rtol=1e-15)


def test_classification_probes_have_a_margin():
    """Where a threshold is not BIG every edge's chi2 is at least 1e-6 (relative) from it, float32 resolution being 6e-8: the classification
    of the device cannot differ from the reference's by rounding.  The strict-compare probes keep that margin for every edge but the
    chosen one, which is 2^-30 from the float32 rounding midpoints instead."""
    for name in pc.CLASSIFICATION_PROBES:
        f, r = pc.probe(name), pc.refs(name).ld
        chosen = pc.strict_edge("seam-257", ps.MONO if "mono" in name else ps.STEREO)[0] if "strict" in name else -1
        for rnd in range(r.rounds):
            th = np.where(f.edge_kind != ps.STEREO, np.float32(f.chi2_mono[rnd]), np.float32(f.chi2_stereo[rnd])).astype(np.longdouble)
            tight = (th < 1e30) & (th > 0) & (np.arange(f.n_edges) != chosen)
            if tight.any():
                assert (np.abs(r.round_chi2[rnd][tight] - th[tight]) / th[tight]).min() > 1e-6, (name, rnd)
    half = pc.refs("seam-257/readmit").ld
    assert 100 < (half.round_chi2[0].astype(np.float32) > np.float32(pc.probe("seam-257/readmit").chi2_mono[0])).sum() < 157


def test_strict_compare_edges():
    for kind, tag in ((ps.MONO, "mono"), (ps.STEREO, "stereo")):
        e, th = pc.strict_edge("seam-257", kind)
        at, below = pc.refs(f"seam-257/strict-{tag}-at"), pc.refs(f"seam-257/strict-{tag}-below")
        for run in (at.ld, at.f64, at.oracle):
            assert run.outlier[e] == 0
        for run in (below.ld, below.f64, below.oracle):
            assert run.outlier[e] == 1
        assert below.ld.n_bad == at.ld.n_bad + 1


def test_seam_and_rig_frames_are_what_they_are_named():
    for n in pc.SEAM_SIZES:
        assert pc.frame(f"seam-{n}").n_edges == n
    rig = pc.frame("rig-1100")
    assert rig.n_edges == 1100 and (rig.edge_kind[1024:] == ps.BODY).sum() > 10 and (rig.edge_kind[1024:] == ps.MONO).sum() > 10
    rot, base = pc.frame("seam-1281-rotated"), pc.frame("seam-1281")
    np.testing.assert_array_equal(rot.points[:200], base.points[1081:])
    assert pc.refs("seam-9/full-big").ld.rounds == 1


def test_reference_iteration_is_quick():
    import time
    f = pc.probe("seam-2809/n1")
    t = time.perf_counter()
    ps.optimize(f, np.longdouble)
    assert time.perf_counter() - t < 1.0
