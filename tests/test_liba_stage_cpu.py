"""CPU validation of tests/liba_stage_numpy.py, the reference side of the inertial stage tests (test_gpu_liba_stages.py,
test_gpu_posei_stages.py): the long-double Schur trial equals a long-double solve of the whole system, noise_floor is
deterministic, and the reference's own float32-record noise stays under the caps that keep a run-time bound from hiding a wrong
Jacobian block (J and the scaled H: 1e-6; b and W r: 5e-6) on every window and frame the GPU tests use.

The GPU tests bound the device by min(2 x noise_floor, cap).  2 x noise_floor is itself under the cap everywhere except: the scaled H
of the one-bias-pair window (floor 7.1e-7: its three robustified links are past the Huber threshold, so rho' = delta / sqrt(chi2)
carries the 1e-7 .. 1e-6 noise of chi2 into every entry of their J^T W J), W r of single links (floors up to 3.2e-6: one of the
fisheye window, a few of the 25-keyframe window) and b of the 60-keyframe map of the GPU file (floor 3.4e-6).  There the cap itself is
the bound, which asks more of the device than the reference's noise would."""
import numpy as np
import pytest

import liba_stage_cases as lc
import liba_stage_numpy as ls


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


@pytest.mark.parametrize("name", ["small_stereo", "no_fixed", "fisheye", "rig", "shared_bias", "some_links", "visual_only"])
def test_schur_route_equals_the_full_long_double_solve(ob, name):
    ls.pn.require_extended()
    w = lc.window(name)
    d = ob.liba_linearize(w)
    lam = lc.default_lambda(d)
    S, bs, x, xl = ls.trial_ld(d["H"], d["b"], d["Hll"], d["Hpl"], w.edge_pose, w.edge_point, w.n_opt, lam)
    xf, xlf = ls.full_solve_ld(d["H"], d["b"], d["Hll"], d["Hpl"], w.edge_pose, w.edge_point, w.n_opt, lam)
    assert S.dtype == np.longdouble and x.dtype == np.longdouble
    assert float(np.abs(x - xf).max() / np.abs(xf).max()) <= 1e-15
    assert float(np.abs(xl - xlf).max() / np.abs(xlf).max()) <= 1e-15


def test_trial_ignores_blocks_of_fixed_keyframes_and_adds_a_rig_pair(ob):
    """The caller's edge order holds edges of fixed keyframes (no keyframe-landmark block) and, for a rig, two edges on one block."""
    w = lc.window("rig")
    d = ob.liba_linearize(w)
    W = ls._landmark_columns(15 * w.n_opt, w.n_opt, d["Hpl"], w.edge_pose, w.edge_point, w.n_points)
    free = w.edge_pose < w.n_opt
    assert (~free).any()
    key = w.edge_pose[free].astype(np.int64) * w.n_points + w.edge_point[free]
    assert len(np.unique(key)) < free.sum()                       # a left + right pair shares its block
    np.testing.assert_allclose(np.asarray(W.sum(axis=(0, 1)), np.float64), d["Hpl"][free].sum(axis=(0, 1)), rtol=1e-12)
    assert np.all(W[:, 6 * w.n_opt:, :] == 0)


def test_noise_floor_is_deterministic_and_moves_only_what_reads_the_record(ob):
    w = lc.window("small_stereo")
    a = ls.noise_floor(lc.liba_system(ob), w, "link_preint", lc.LIBA_MEASURES)
    b = ls.noise_floor(lc.liba_system(ob), w, "link_preint", lc.LIBA_MEASURES)
    assert a == b
    assert a["Hll"] == 0.0 and a["Hpl"] == 0.0 and a["bl"] == 0.0     # no float32 getter on the visual side
    assert a["H"] > 0.0 and a["b"] > 0.0
    p = ls.perturbed(w, "link_preint", 0)
    assert p.link_preint.dtype == np.float32 and p.link_preint is not w.link_preint
    nz = w.link_preint != 0
    ulp = np.abs(np.spacing(w.link_preint[nz]))
    assert np.all(np.abs(p.link_preint[nz] - w.link_preint[nz]) <= ulp) and np.all(p.link_preint[nz] != w.link_preint[nz])


@pytest.mark.parametrize("name", lc.WINDOWS)
def test_window_noise_stays_under_the_caps(ob, name):
    w = lc.window(name)
    nf = ls.noise_floor(lc.liba_system(ob), w, "link_preint", lc.LIBA_MEASURES)
    print(f"\n{name}: " + " ".join(f"{k} {v:.2e}" for k, v in nf.items()))
    assert nf["H"] <= lc.CAP_H and nf["b"] <= lc.CAP_B
    if name != "shared_bias":
        assert 2 * nf["H"] <= lc.CAP_H
    assert 2 * nf["b"] <= lc.CAP_B
    assert nf["Hll"] == 0.0 and nf["Hpl"] == 0.0 and nf["bl"] == 0.0
    if w.n_links:
        ne = ls.noise_floor(lc.liba_links(ob), w, "link_preint")
        print("   links: " + " ".join(f"{k} {v:.2e}" for k, v in ne.items()))
        assert 2 * max(v for k, v in ne.items() if k.startswith("J")) <= lc.CAP_H
        assert max(v for k, v in ne.items() if not k.startswith("J")) <= lc.CAP_B


@pytest.mark.parametrize("name", lc.FRAMES)
def test_frame_noise_stays_under_the_caps(ob, name):
    f = lc.frame(name)
    nf = ls.noise_floor(lc.posei_system(ob), f, "preint", lc.POSEI_MEASURES)
    print(f"\n{name}: " + " ".join(f"{k} {v:.2e}" for k, v in nf.items()))
    assert 2 * nf["H"] <= lc.CAP_H and 2 * nf["b"] <= lc.CAP_B
