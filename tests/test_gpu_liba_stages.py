"""Stage-by-stage GPU checks of the inertial bundle adjustment kernel (k_liba, csrc/liba_device.hip): one linearisation and one trial
per case, never a Levenberg-Marquardt run.

  visual blocks   Hll, Hpl, b_l (and everything of a window without links) against the oracle at the LBA suite's own numbers
                  (test_gpu_lba.py:_assert_blocks): 1e-11 of the array's largest entry, 1e-10 for fisheye.  No float32 getter there.
  link forms      J, -rho' W r, rho' of every link (osh_liba_inertial_edges) against the oracle's liba_inertial_edge.
  the system      H, b, chi2 (osh_liba_linearize) against the oracle's liba_linearize; H as |dH_ij| / sqrt(H_ii H_jj).
                  Bound: min(2 x noise_floor, cap) of the same quantity on the same window, computed at run time
                  (liba_stage_numpy.noise_floor: the ORACLE's own change under one float32 ulp of the preintegration record; caps
                  1e-6 for J and the scaled H, 5e-6 for b and W r -- see test_liba_stage_cpu.py for where the cap is the smaller).
  default lambda  lambda_used of osh_liba_debug_trial(lambda = 0) against kLmTau x the largest diagonal entry of the oracle's system.
  one trial       S, bs, x, landmark step against the np.longdouble trial (liba_stage_numpy.trial_ld) of the DEVICE's own H, b, Hll,
                  Hpl: Schur + LDL^T + back-substitution on their own.  S, bs to 1e-12 of the largest entry; x to 1e-6 relative
                  and no worse than 10 x float64 numpy's own distance.
  the update      osh_liba_solve(max_iterations = 1) against liba_numpy.State.oplus of the device's own step, 64 x 2^-53.

Every case asserts the path it means to take from `info` (NB, G, C, il, n_colours).

Measured on an MI355X, device distance | bound (the tests print these lines with -s; G = 32 unless noted):
    case          NB  C il colours   scaled H               b                      chi2                   links worst/bound (J, W r, rho')
    small_stereo  24  8  0   2       1.19e-09 | 3.58e-07   4.58e-09 | 1.13e-06   2.02e-09 | 1.54e-06   0.05 0.01 0.00
    no_fixed      24  8  0   2       1.17e-09 | 3.58e-07   3.89e-09 | 1.22e-06   6.19e-10 | 1.54e-06   0.05 0.01 0.00
    fisheye       24  8  0   2       4.62e-11 | 3.58e-07   8.63e-09 | 2.32e-06   3.77e-10 | 2.14e-06   0.00 0.00 0.00
    rig           24  8  0   2       1.18e-09 | 3.58e-07   6.02e-09 | 1.64e-06   4.99e-10 | 1.04e-06   0.05 0.01 0.01
    shared_bias   24  8  0   4       5.57e-08 | 1.00e-06   3.43e-09 | 8.12e-07   5.60e-11 | 2.08e-07   0.05 0.00 0.00   (rho' < 1 at 3 links)
    some_links    24  8  0   2       1.19e-09 | 3.58e-07   6.90e-09 | 1.39e-06   2.66e-09 | 2.13e-06   0.05 0.01 0.00
    visual_only   24  8  0   0       4.42e-16 | 1.00e-11   1.19e-16 | 1.00e-11   2.02e-16 | 1.00e-11   -
    lds_panels    24  3  0   2       8.46e-10 | 3.58e-07   6.11e-09 | 1.46e-06   1.96e-10 | 4.45e-07   0.05 0.01 0.01   (same with G = 1, C = 1)
    eight_chunks  24  8  0   2       1.13e-09 | 3.58e-07   7.14e-09 | 2.77e-06   9.59e-10 | 1.49e-06   -                (same with G = 1, C = 1)
    banded         6  1  1   2       1.75e-09 | 3.62e-07   7.12e-08 | 5.00e-06   1.19e-09 | 1.17e-06   0.05 0.03 0.00
  Hll, b_l, Hpl: 2e-16 .. 1.4e-14 of the largest entry everywhere (bound 1e-11, fisheye 1e-10).  Every case but visual_only has a
  robustified link past the Huber threshold (rho' 0.003 .. 0.05).
  One trial against long double: S and bs 1e-17 .. 1.4e-15 (bound 1e-12); keyframe step 4e-15 .. 1.7e-13 with float64 numpy at
  4e-15 .. 1.7e-13 on the same systems; landmark step 6e-15 .. 2e-13 (numpy 1e-14 .. 4e-13).  The default lambda equals the oracle's to
  7 digits and more (2.128025e+05 on the stereo windows).  Update: 2.7 .. 4 x 2^-53 (bound 64).

Sensitivity (scratch builds, not committed): one bias-Jacobian block (dV/dbg of inertial_residual_jacobian) scaled by 1 + 1e-4 passes
all of test_gpu_liba.py and fails every case here that has a link; one pose-row chunk dropped from S where C > 1 fails 15 tests of
test_gpu_liba.py and, here, the cases whose dropped chunk holds edges (lds_panels, eight_chunks).
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import liba_stage_cases as lc
import liba_stage_numpy as ls
from oracle import liba_numpy as ln
from orb_slam3_study_kr_amd import capi, lba
from orb_slam3_study_kr_amd import synth_inertial as si

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def solver(hip_lib):
    ls.pn.require_extended()
    with lba.LbaSolver(0) as s:
        yield s


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


def _banded():
    """The smallest map of this generator that takes the banded layout: 60 keyframes half a second apart (a landmark is seen over at
    most 29 of them; with 59 the band is no longer under half the system and the layout stays dense)."""
    return si.make_inertial_window(905, n_opt=60, n_fixed=0, n_points=400, large=True, kf_dt=0.5)


def _window(name):
    return _banded() if name == "banded" else lc.window(name)


_refs = {}


def _reference(ob, name):
    """(oracle system, noise floors of the system, noise floors of the link forms) of a case, computed once."""
    if name not in _refs:
        w = _window(name)
        _refs[name] = (ob.liba_linearize(w), ls.noise_floor(lc.liba_system(ob), w, "link_preint", lc.LIBA_MEASURES),
                       ls.noise_floor(lc.liba_links(ob), w, "link_preint") if w.n_links else {})
    return _refs[name]


def _bound(floor, cap, tol=1e-11):
    """2 x the reference's float32 noise, never above the cap (or it could hide a wrong block) and never below the float64 number of the
    visual blocks (a quantity the record's noise does not reach still carries the rounding of another order of float64 sums)."""
    return max(min(2 * floor, cap), tol)


def _pair_sum(w, Hpl):
    """Hpl summed per (keyframe, landmark) block: the two edges of a rig's left + right pair share one."""
    key = w.edge_pose.astype(np.int64) * w.n_points + w.edge_point
    u, inv = np.unique(key, return_inverse=True)
    out = np.zeros((len(u), 6, 3))
    np.add.at(out, inv, np.where((w.edge_pose < w.n_opt)[:, None, None], Hpl, 0.0))
    return out


def _assert_system(name, w, got, ref, nf):
    n = 15 * w.n_opt
    tol = 1e-10 if w.kb8 is not None else 1e-11
    vis = dict(Hll=(got["Hll"], ref["Hll"]), bl=(got["b"][n:], ref["b"][n:]), Hpl=(_pair_sum(w, got["Hpl"]), _pair_sum(w, ref["Hpl"])))
    for k, (a, b) in vis.items():
        d = ls.rel_max(a, b)
        print(f"    {name:12s} {k:4s} {d:.2e} | {tol:.0e}")
        assert d <= tol, (name, k, d)
    # (a window without links: nothing reads a float32 record, the floors are 0 and the visual number holds for all of it)
    bound_h, bound_b, bound_c = _bound(nf["H"], lc.CAP_H, tol), _bound(nf["b"], lc.CAP_B, tol), _bound(nf["chi2"], lc.CAP_B, tol)
    dh, db, dc = ls.scaled_h(got["H"], ref["H"]), ls.rel_max(got["b"][:n], ref["b"][:n]), ls.rel_scalar(got["chi2"], ref["chi2"])
    print(f"    {name:12s} scaled H {dh:.2e} | {bound_h:.2e}   b {db:.2e} | {bound_b:.2e}   chi2 {dc:.2e} | {bound_c:.2e}   {got['info']}")
    assert dh <= bound_h and db <= bound_b and dc <= bound_c, (name, dh, bound_h, db, bound_b, dc, bound_c)


def _assert_links(name, w, ob, solver, ne):
    J, Wr, rho1 = solver.inertial_edges(w)
    worst = [0.0, 0.0, 0.0]
    n_soft = 0
    for l in range(w.n_links):
        Jr, Wrr, rr, chi = lc.link_forms(ob, w, l)
        n_soft += rr < 1.0
        bj, bw, br = _bound(ne[f"J{l}"], lc.CAP_H), _bound(ne[f"Wr{l}"], lc.CAP_B), _bound(ne[f"rho{l}"], lc.CAP_B)
        sj = np.abs(Jr).max()
        dj = max(np.abs(J[l][:, 3 * c:3 * c + 3] - Jr[:, 3 * c:3 * c + 3]).max() for c in range(8)) / sj      # per 3 x 3 block column
        dw = ls.rel_max(Wr[l], rr * Wrr)
        dr = abs(rho1[l] - rr) / rr
        worst = [max(worst[0], dj / bj), max(worst[1], dw / bw), max(worst[2], dr / br)]
        assert dj <= bj and dw <= bw and dr <= br, (name, l, dj, bj, dw, bw, dr, br)
    print(f"    {name:12s} links {w.n_links}, rho' < 1 at {n_soft}: worst distance / bound  J {worst[0]:.2f}  W r {worst[1]:.2f}  rho' {worst[2]:.2f}")
    return n_soft


def _assert_trial(name, w, solver, got, ref):
    """One trial at the default lambda, against the long-double trial of the device's own system."""
    S, bs, x, xl, lam = solver.debug_trial_inertial(w, 0.0)
    return _assert_trial_of(name, w, got, ref, S, bs, x, xl, lam)


def _assert_trial_of(name, w, got, ref, S, bs, x, xl, lam):
    lam_ref = lc.default_lambda(ref)
    S_ld, bs_ld, x_ld, xl_ld = ls.trial_ld(got["H"], got["b"], got["Hll"], got["Hpl"], w.edge_pose, w.edge_point, w.n_opt, lam)
    ds, dbs = float(np.abs(S - S_ld).max() / np.abs(S_ld).max()), float(np.abs(bs - bs_ld).max() / np.abs(bs_ld).max())
    x64 = np.linalg.solve(np.asarray(S_ld, np.float64), np.asarray(bs_ld, np.float64))
    sx = float(np.abs(x_ld).max())
    dx, d64 = float(np.abs(x - x_ld).max()) / sx, float(np.abs(x64 - x_ld).max()) / sx
    # the landmark step comes back as (trial point - point): one rounding of the point's magnitude on top of the step's own error;
    # numpy's own distance here is that of the whole trial done in float64
    xl64 = ls.trial_ld(got["H"], got["b"], got["Hll"], got["Hpl"], w.edge_pose, w.edge_point, w.n_opt, lam, dtype=np.float64)[3]
    sl = float(np.abs(xl_ld).max())
    dl, dl64 = float(np.abs(xl - xl_ld).max()) / sl, float(np.abs(xl64 - xl_ld).max()) / sl
    round_l = 2 * U53 * float(np.abs(w.points).max()) / sl
    print(f"    {name:12s} lambda {lam:.6e} (oracle {lam_ref:.6e})  S {ds:.2e}  bs {dbs:.2e} | 1e-12   x device {dx:.2e} numpy {d64:.2e}   "
          f"landmarks device {dl:.2e} numpy {dl64:.2e} (rounding of the points {round_l:.1e})")
    assert ds <= 1e-12 and dbs <= 1e-12, (name, ds, dbs)
    assert dx <= 1e-6 and dx <= 10 * max(d64, U53), (name, dx, d64)
    assert dl <= 1e-6 and dl <= 10 * max(dl64, U53) + round_l, (name, dl, dl64, round_l)
    return lam, lam_ref


CASES = ["small_stereo", "no_fixed", "fisheye", "rig", "shared_bias", "some_links", "visual_only", "lds_panels", "banded"]


@pytest.mark.parametrize("name", CASES)
def test_first_system_link_forms_and_one_trial(solver, ob, name):
    w = _window(name)
    ref, nf, ne = _reference(ob, name)
    got = solver.linearize_inertial(w)
    info = got["info"]
    print()
    # ---- the path this case is here for
    assert info["G"] == 32 and info["C"] == max(1, min(8, (128 - 32) // w.n_opt))
    assert (info["NB"], info["il"]) == ((6, 1) if name == "banded" else (24, 0))
    if name == "shared_bias":
        assert info["n_colours"] >= 3                    # every link shares the bias keyframe with every other
    elif name == "visual_only":
        assert w.n_links == 0 and info["n_colours"] == 0
    else:
        assert info["n_colours"] == min(2, w.n_links)    # a chain of links takes two colours
    if name == "rig":
        key = w.edge_pose.astype(np.int64) * w.n_points + w.edge_point
        assert len(np.unique(key)) < w.n_edges           # left + right pairs on one block
    _assert_system(name, w, got, ref, nf)
    if w.n_links:
        n_soft = _assert_links(name, w, ob, solver, ne)
        if name == "shared_bias":
            assert n_soft >= 1                           # a robustified link past the Huber threshold: rho' < 1
    lam, lam_ref = _assert_trial(name, w, solver, got, ref)
    bound_lam = _bound(nf["H"], lc.CAP_H)
    assert abs(lam - lam_ref) <= bound_lam * lam_ref, (name, lam, lam_ref)


@pytest.mark.parametrize("group,chunks", [("1", 1), ("32", 8)])
@pytest.mark.parametrize("name", ["small_stereo", "lds_panels", "eight_chunks"])
def test_group_sizes_and_pose_row_chunks(solver, ob, monkeypatch, name, group, chunks):
    """One block per window sums a pose row in one chunk, a group of 32 in up to 8 (3 keyframes: 8; 25 keyframes: 3).  The 80-landmark
    window fills only two of its eight chunks; `eight_chunks` and the 25-keyframe window fill every chunk of every pose row, so a
    chunk that is dropped or read twice anywhere (S, the right-hand side, the default lambda, the export's own sum) shows."""
    monkeypatch.setenv("OSH_LIBA_GROUP", group)
    w = _window(name)
    ref, nf, ne = _reference(ob, name)
    got = solver.linearize_inertial(w)
    want_c = (1 if group == "1" else 3) if name == "lds_panels" else chunks
    assert (got["info"]["G"], got["info"]["C"]) == (int(group), want_c), got["info"]
    if name != "small_stereo":
        assert lc.chunk_occupancy(w, want_c) == [want_c] * w.n_opt
    print()
    _assert_system(name, w, got, ref, nf)
    _assert_trial(name, w, solver, got, ref)


def test_banded_and_dense_layout_of_one_map_give_the_same_stages(solver, monkeypatch):
    """OSH_LIBA_DENSE=1 keeps the [poses | velocities, biases] order for the map that otherwise takes the interleaved banded one: the
    linearisation adds the same terms in the same order (equal bits, only their place differs), the Schur sums and the elimination run
    in another order (S to 1e-12 as against long double, the step to 1e-9: both are within 1e-12 of the refined solve above)."""
    w = _window("banded")
    a = solver.linearize_inertial(w)
    ta = solver.debug_trial_inertial(w, 0.0)
    monkeypatch.setenv("OSH_LIBA_DENSE", "1")
    b = solver.linearize_inertial(w)
    tb = solver.debug_trial_inertial(w, 0.0)
    assert (a["info"]["il"], b["info"]["il"]) == (1, 0) and a["info"]["NB"] == b["info"]["NB"] == 6
    for k in ("H", "b", "Hll", "Hpl"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert ta[4] == tb[4]
    assert ls.rel_max(ta[0], tb[0]) <= 1e-12 and ls.rel_max(ta[1], tb[1]) <= 1e-12
    assert ls.rel_max(ta[2], tb[2]) <= 1e-9 and ls.rel_max(ta[3], tb[3]) <= 1e-9


def test_a_given_lambda_is_used_as_given(solver, ob):
    w = _window("no_fixed")
    got = solver.linearize_inertial(w)
    S, bs, x, xl, lam = solver.debug_trial_inertial(w, 3.5)
    assert lam == 3.5
    print()
    _assert_trial_of("no_fixed", w, got, _reference(ob, "no_fixed")[0], S, bs, x, xl, lam)


@pytest.mark.parametrize("name", ["small_stereo", "fisheye", "rig", "shared_bias"])
def test_update_of_an_accepted_trial(solver, name):
    """The state after one accepted trial = oplus of the device's own step (ImuCamPose::Update, the velocity / bias and point sums)."""
    w = dataclasses.replace(_window(name), lambda_init=1e-2, max_iterations=1)
    S, bs, x, xl, lam = solver.debug_trial_inertial(w, 1e-2)
    res = solver.solve_inertial([w])[0]
    assert res.iterations == 1 and list(res.trials_trace) == [1]          # the first trial was accepted
    st = ln.State(w)
    st.oplus(np.concatenate([x, xl.ravel()]))
    N = w.n_opt
    worst = 0.0
    for fld, exp in (("pose_Rwb", st.Rwb[:N]), ("pose_twb", st.twb[:N]), ("pose_Rcw", st.Rcw[:N]), ("pose_tcw", st.tcw[:N]), ("vel", st.vel[:N]),
                     ("bias_g", st.bg[:N]), ("bias_a", st.ba[:N]), ("points", st.X)):
        got = np.asarray(getattr(res, fld)).reshape(exp.shape)
        mag = max(1.0, np.abs(exp).max()) if fld.startswith("pose_R") else np.abs(exp).max()
        d = np.abs(got - exp).max() / mag
        worst = max(worst, d)
        assert d <= 64 * U53, (name, fld, d)
    print(f"\n    {name:12s} update: worst distance {worst / U53:.1f} x 2^-53 | 64")


def test_refusals(solver):
    w = _window("small_stereo")
    n, L, E, NL = 15 * w.n_opt, w.n_points, w.n_edges, w.n_links
    d = capi.c_double_p
    H, b, Hll, Hpl, chi = np.zeros((n, n)), np.zeros(n + 3 * L), np.zeros((L, 3, 3)), np.zeros((E, 6, 3)), np.zeros(1)
    info = np.zeros(5, dtype=np.int32)
    lib, ctx = solver.lib, solver.ctx
    full = [capi.ptr(H, d), capi.ptr(b, d), capi.ptr(Hll, d), capi.ptr(Hpl, d), capi.ptr(chi, d), capi.ptr(info, capi.c_int32_p)]
    p = w.as_struct()
    for k in range(len(full)):
        args = list(full)
        args[k] = None
        assert lib.osh_liba_linearize(ctx, C.byref(p), *args) == capi.OSH_ERR_INVALID, k
    assert lib.osh_liba_linearize(ctx, None, *full) == capi.OSH_ERR_INVALID
    J, Wr, r1 = np.zeros((NL, 9, 24)), np.zeros((NL, 9)), np.zeros(NL)
    assert lib.osh_liba_inertial_edges(ctx, C.byref(p), None, capi.ptr(Wr, d), capi.ptr(r1, d)) == capi.OSH_ERR_INVALID
    assert lib.osh_liba_inertial_edges(ctx, C.byref(p), capi.ptr(J, d), capi.ptr(Wr, d), None) == capi.OSH_ERR_INVALID
    S, bs, x, xl, lam = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros((L, 3)), np.zeros(1)
    assert lib.osh_liba_debug_trial(ctx, C.byref(p), 1.0, capi.ptr(S, d), capi.ptr(bs, d), capi.ptr(x, d), None, capi.ptr(lam, d)) == capi.OSH_ERR_INVALID
    assert lib.osh_liba_debug_trial(ctx, C.byref(p), 1.0, capi.ptr(S, d), capi.ptr(bs, d), capi.ptr(x, d), capi.ptr(xl, d), None) == capi.OSH_ERR_INVALID
    # sizes and indices out of range
    for fld, val in (("n_opt", 0), ("n_fixed_imu", 2), ("n_edges", -1), ("n_links", -1)):
        q = w.as_struct()
        setattr(q, fld, val)
        assert lib.osh_liba_linearize(ctx, C.byref(q), *full) == capi.OSH_ERR_INVALID, fld
    bad = dataclasses.replace(w, edge_pose=np.where(np.arange(E) == 7, w.n_opt + w.n_fixed_imu + w.n_fixed, w.edge_pose).astype(np.int32))
    q = bad.as_struct()
    assert lib.osh_liba_linearize(ctx, C.byref(q), *full) == capi.OSH_ERR_INVALID
    bad = dataclasses.replace(w, link_cur=np.where(np.arange(NL) == 1, w.n_opt, w.link_cur).astype(np.int32))
    q = bad.as_struct()
    assert lib.osh_liba_inertial_edges(ctx, C.byref(q), capi.ptr(J, d), capi.ptr(Wr, d), capi.ptr(r1, d)) == capi.OSH_ERR_INVALID
    # and the context is fine afterwards
    assert solver.linearize_inertial(w)["info"]["G"] == 32
