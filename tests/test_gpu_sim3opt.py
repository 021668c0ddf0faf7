"""Optimizer::OptimizeSim3 on the device (osh_sim3_optimize / osh_sim3_linearize / the host entry point) against sim3opt_numpy."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import pgo_numpy as pn
import sim3opt_numpy as sn
from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_sim3 as ss
from orb_slam3_study_kr_amd.lba import LbaSolver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    with LbaSolver(0) as s:
        yield s


def _rot_err(qa, qb):
    d = pn.quat_mul(np.asarray(qa), np.concatenate([-np.asarray(qb)[:3], np.asarray(qb)[3:4]]))
    return 2 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))


@pytest.mark.parametrize("n,seed", [(30, 1), (300, 2), (1500, 3)])
def test_first_linearization_matches_numpy(solver, n, seed):
    pk = ss.pack(ss.make_case(seed, n, 0.2, n_no_i2=3))
    chi, H, b = solver.linearize_sim3(pk)
    chi_np, H_np, b_np, _, _ = sn.linearize(pk, pk["S12"], np.ones(len(pk["index"]), bool), True)
    assert abs(chi - chi_np) <= 1e-14 * abs(chi_np)
    assert np.abs(H - H_np).max() <= 1e-8 * np.abs(H_np).max()
    assert np.abs(b - b_np).max() <= 1e-8 * np.abs(b_np).max()


def _th_close(pk, c12, c21):
    th = float(np.float32(pk["th2"]))
    return (np.abs(c12 - th) <= 1e-6 * th) | (np.abs(c21 - th) <= 1e-6 * th)


CASES = [(n, frac, no_i2, fs) for n in (30, 300, 1500) for frac in (0.0, 0.2, 0.4) for no_i2 in (0, 5) for fs in (False, True)]


@pytest.mark.parametrize("n,frac,no_i2,fix_scale", CASES)
def test_pinhole_matches_numpy(solver, n, frac, no_i2, fix_scale):
    seed = n * 7 + int(frac * 10) + no_i2 + 100 * fix_scale
    pk = ss.pack(ss.make_case(seed, n, frac, n_no_i2=no_i2, fix_scale=fix_scale))
    dev = solver.optimize_sim3([pk])[0]
    ref = sn.run(pk)
    assert dev.round2 == ref.round2
    for k, rr in enumerate(ref.rounds):
        # exact, except where numpy's last gain sits at a stop rule, whose outcome then depends on the order of the sums: +-1 at or
        # below the 1e-3 rule (whether a trial of relative gain ~1e-8 is accepted); on an estimate converged to rounding level
        # (gain ~1e-16) one side may stop at once on rho == 0 while the other counts three bad iterations, a difference of 2
        slack = 2 if abs(rr.last_gain) < 1e-12 else 1 if rr.last_gain < 1.1e-3 else 0
        assert abs(dev.iterations[k] - rr.iterations) <= slack, (k, dev.iterations, ref.iterations)
    amb = _th_close(pk, ref.chi2_12, ref.chi2_21) | _th_close(pk, dev.chi2_12, dev.chi2_21)
    assert np.array_equal(dev.outlier1[~amb], ref.outlier1[~amb])
    assert np.array_equal(dev.outlier[~amb], ref.outlier[~amb])
    assert abs(dev.n_in - ref.n_in) <= int(amb.sum())
    assert dev.n_bad == int(dev.outlier1.sum())
    if ref.round2:
        assert _rot_err(dev.S12[:4], ref.S12[:4]) < 1e-6
        assert np.linalg.norm(dev.S12[4:7] - ref.S12[4:7]) <= 1e-6 * np.linalg.norm(ref.S12[4:7])
        assert abs(dev.S12[7] - ref.S12[7]) <= 1e-6 * ref.S12[7]
    if fix_scale:
        assert dev.S12[7] == pk["S12"][7]


@pytest.mark.parametrize("fix_scale", [False, True])
def test_kannala_brandt8(solver, fix_scale):
    pk = ss.pack(ss.make_case(41 + fix_scale, 300, 0.2, n_no_i2=3, kb8=True, fix_scale=fix_scale))
    chi, _, _ = solver.linearize_sim3(pk)
    chi_np, _, _, _, _ = sn.linearize(pk, pk["S12"], np.ones(len(pk["index"]), bool), True)
    assert abs(chi - chi_np) <= 1e-12 * abs(chi_np)
    dev = solver.optimize_sim3([pk])[0]
    assert dev.round2
    act = dev.outlier1 == 0
    bad, n_in = sn.classify(pk, dev.S12, act)
    assert dev.n_in == n_in
    assert np.array_equal(dev.outlier.astype(bool), dev.outlier1.astype(bool) | bad)
    # the device's estimate is no worse than the initial one over the final inliers (plain chi2)
    ini, _, _ = sn.active_chi2(pk, pk["S12"], act, False)
    fin, _, _ = sn.active_chi2(pk, dev.S12, act, False)
    assert fin <= ini
    if fix_scale:
        assert dev.S12[7] == pk["S12"][7]


def test_early_return_keeps_s12_and_reports_round1(solver):
    pk = ss.pack(ss.make_case(77, 14, 0.6))
    dev = solver.optimize_sim3([pk])[0]
    ref = sn.run(pk)
    assert not ref.round2 and not dev.round2
    assert dev.n_in == 0 and dev.iterations[1] == 0
    assert np.array_equal(dev.S12, pk["S12"])
    assert dev.n_bad > 0 and np.array_equal(dev.outlier, dev.outlier1)
    assert np.array_equal(dev.outlier1, ref.outlier1)


def test_batch_equals_single(solver):
    packs = []
    for k in range(16):
        packs.append(ss.pack(ss.make_case(300 + k, [30, 300, 800, 12][k % 4], [0.0, 0.2, 0.4, 0.6][k % 4], n_no_i2=k % 3,
                                          fix_scale=k % 2 == 1, kb8=k % 5 == 0)))
    batch = solver.optimize_sim3(packs)
    for pk, b in zip(packs, batch):
        s = solver.optimize_sim3([pk])[0]
        assert np.array_equal(s.S12, b.S12)
        for f in ("outlier1", "outlier", "chi2_12", "chi2_21"):
            assert np.array_equal(getattr(s, f), getattr(b, f)), f
        assert (s.n_bad, s.n_in, s.round2, s.iterations, s.chi2_end) == (b.n_bad, b.n_in, b.round2, b.iterations, b.chi2_end)


def _host_call(case, hessian):
    lib = capi.load_host_library()
    inp = ss.host_input(case)
    nulled = np.zeros(len(case.matches1), np.uint8)
    S = np.zeros(8)
    H = np.ascontiguousarray(hessian, np.float64).copy()
    ret = lib.osh_host_optimize_sim3(C.byref(inp), capi.ptr(nulled, capi.c_uint8_p), capi.ptr(S, capi.c_double_p),
                                     capi.ptr(H, capi.c_double_p))
    return ret, nulled, S, H


@pytest.mark.parametrize("kw", [dict(), dict(fix_scale=True), dict(all_points=False), dict(kb8=True)])
def test_optimize_sim3_entry_point(solver, kw):
    case = ss.make_case(500 + len(kw), 400, 0.2, n_no_i2=6, n_bad=6, n_null_mp1=4, n_neg_depth=4, **kw)
    pk = ss.pack(case)
    dev = solver.optimize_sim3([pk])[0]
    ret, nulled, S, H = _host_call(case, np.full(49, 7.0))
    assert ret == dev.n_in and dev.round2
    expect = np.zeros(len(case.matches1), np.uint8)
    expect[pk["index"][dev.outlier.astype(bool)]] = 1
    assert np.array_equal(nulled, expect)
    assert np.array_equal(S, dev.S12)
    assert np.all(H == 0.0)
    # bad points and NULL pMP1 slots are never nulled
    m = case.matches1
    bad = np.array([i for i in range(len(m)) if m[i] >= 0 and (case.kf1_mp[i] < 0 or case.mp_bad[case.kf1_mp[i]] or case.mp_bad[m[i]])])
    assert len(bad) > 0 and not nulled[bad].any()


def test_optimize_sim3_entry_point_early_return():
    case = ss.make_case(77, 14, 0.6)
    pk = ss.pack(case)
    ref = sn.run(pk)
    assert not ref.round2
    H0 = np.arange(49, dtype=np.float64)
    ret, nulled, S, H = _host_call(case, H0)
    assert ret == 0
    assert np.array_equal(S, np.asarray(case.S12, np.float64))
    assert np.array_equal(H, H0)
    expect = np.zeros(len(case.matches1), np.uint8)
    expect[pk["index"][ref.outlier1.astype(bool)]] = 1
    assert np.array_equal(nulled, expect) and nulled.any()
