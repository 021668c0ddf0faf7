"""GPU checks of the 4-DoF pose graph of OptimizeEssentialGraph4DoF (osh_pgo4_*, csrc/pgo4_device.hip) against the FP64 numpy
restatement in pgo4_numpy.py, on synthetic inertial loops (synth_pgo.make_inertial_loop / pack_loop4)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import pgo4_numpy as p4
from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_pgo as sp
from orb_slam3_study_kr_amd.pgo import Pgo4Graph, PgoSolver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    with PgoSolver(0) as s:
        yield s


def _graph(n, earlier=False, seed=7, rp=0.001):
    m = sp.make_inertial_loop(n, seed=seed, earlier_loop=earlier, rp_noise=rp)
    g, _, _ = sp.pack_loop4(m)
    return g


@pytest.mark.parametrize("n", [50, 300])
def test_first_linearization_matches_numpy(solver, n):
    g = _graph(n, earlier=n == 300)
    chi2, H, b = solver.linearize4(g)
    chi2_ref, H_ref, b_ref = p4.linearize(g)
    # chi2 at the raw camera poses (no vertex has been updated yet)
    assert np.isclose(chi2, chi2_ref, rtol=1e-12)
    nf = H.shape[0] // 4
    assert nf == int(np.count_nonzero(~g.fixed))
    for a in range(nf):
        cols = np.flatnonzero(np.abs(H_ref[4 * a:4 * a + 4]).reshape(4, nf, 4).max(axis=(0, 2)) > 0)
        assert np.all(H[4 * a:4 * a + 4].reshape(4, nf, 4)[:, np.setdiff1d(np.arange(nf), cols)] == 0)
        for c in cols:
            blk, ref = H[4 * a:4 * a + 4, 4 * c:4 * c + 4], H_ref[4 * a:4 * a + 4, 4 * c:4 * c + 4]
            assert np.abs(blk - ref).max() <= 1e-7 * np.abs(ref).max(), (a, c)
        bs, br = b[4 * a:4 * a + 4], b_ref[4 * a:4 * a + 4]
        assert np.abs(bs - br).max() <= 1e-7 * max(np.abs(br).max(), 1e-9), a


CASES = [(50, False), (50, True), (300, False), (300, True), (1000, False), (1000, True)]


@pytest.mark.parametrize("n,earlier", CASES)
def test_optimize_matches_numpy(solver, n, earlier):
    g = _graph(n, earlier)
    r = solver.solve4(g)
    ref = p4.optimize(g)
    assert (r.iterations, r.trials) == (ref.iterations, ref.trials)
    assert np.isclose(r.lambda_init_used, ref.lambda_init, rtol=1e-9)
    assert np.isclose(r.chi2_initial, ref.chi2_initial, rtol=1e-12)
    assert np.isclose(r.chi2_final, ref.chi2_final, rtol=1e-6)
    assert r.chi2_final < 0.2 * r.chi2_initial
    # the Sim3 graph's bounds: 1.2e-5 in rotation, 7e-6 of the largest translation
    assert np.abs(r.Rcw - ref.state["Rcw"]).max() <= 1.2e-5
    assert np.abs(r.tcw - ref.state["tcw"]).max() <= 7e-6 * np.abs(ref.state["tcw"]).max()
    if n == 300:
        # six or more accepted steps: the DR normalisation ran in a step and in the perturbed evaluations that followed
        assert ref.max_its_updates >= 6


@pytest.mark.parametrize("n,earlier", [(300, True), (1000, False)])
def test_only_yaw_and_translation_move(solver, n, earlier):
    """Rwb = DR Rwb0 with DR a rotation about world z: row 2 of Rwb (the world z axis seen from the body) does not move, and
    the fixed pLoopKF keeps its raw pose byte for byte."""
    g = _graph(n, earlier)
    r = solver.solve4(g)
    assert np.abs(r.Rwb[:, 2, :] - g.Rwb[:, 2, :]).max() <= 1e-12
    assert np.abs(r.Rwb[:, :2, :] - g.Rwb[:, :2, :]).max() > 1e-4          # yaw did move
    f = np.flatnonzero(g.fixed)
    assert len(f) == 1
    assert r.Rcw[f].tobytes() == np.ascontiguousarray(g.Rcw[f]).tobytes()
    assert r.tcw[f].tobytes() == np.ascontiguousarray(g.tcw[f]).tobytes()


def test_envelope_equals_dense(solver):
    # one LM iteration: the first trial's step comes from the same system through the envelope and the full upper triangle
    g = _graph(400, earlier=True)
    env = solver.solve4(g, iterations=1)
    dense = solver.solve4(g, iterations=1, dense=True)
    assert env.tall_columns > 0 and env.envelope_tiles < dense.envelope_tiles
    assert (env.iterations, env.trials) == (dense.iterations, dense.trials) == (1, 1)
    assert np.abs(env.tcw - g.tcw).max() > 1e-3     # the step was taken
    assert np.abs(env.Rcw - dense.Rcw).max() <= 1e-10
    assert np.abs(env.tcw - dense.tcw).max() <= 1e-10 * np.abs(dense.tcw).max()


def test_deterministic_and_independent_of_arena_history():
    from orb_slam3_study_kr_amd import lba, synth
    g = _graph(300, earlier=True)
    with PgoSolver(0) as fresh:
        a = fresh.solve4(g)
        b = fresh.solve4(g)
    assert a.Rcw.tobytes() == b.Rcw.tobytes() and a.tcw.tobytes() == b.tcw.tobytes()
    # a context that has just run a global BA and a Sim3 graph
    with lba.LbaSolver(0) as s:
        w = synth.make_window(5, n_free=300, n_fixed=1, n_points=6000, stereo=False)
        s.solve([w])
        ps = PgoSolver.__new__(PgoSolver)
        ps.lib, ps.ctx = s.lib, s.ctx
        g3, _, _ = sp.pack_loop(sp.make_map(1000, seed=3, mono=True, earlier_loop=True))
        ps.solve(g3)
        c = ps.solve4(g)
    assert c.Rcw.tobytes() == a.Rcw.tobytes() and c.tcw.tobytes() == a.tcw.tobytes()
    assert (c.iterations, c.trials, c.chi2_final) == (a.iterations, a.trials, a.chi2_final)


def test_lambda_init_rule(solver):
    g = _graph(50)
    _, H, _ = solver.linearize4(g)
    r = solver.solve4(g, lambda_init=0.0)
    assert r.lambda_init_used == 1e-5 * np.abs(np.diag(H)).max()
    u = solver.solve4(g, lambda_init=3.5)
    assert u.lambda_init_used == 3.5
    assert u.Rcw.tobytes() != r.Rcw.tobytes()


def _refused(solver, g, expect, lambda_init=0.0, mutate=None):
    prob = g.as_struct(20, lambda_init)
    if mutate:
        mutate(prob)
    sentinel = np.full(9 * max(len(g.fixed), 1), 7.0)
    res = capi.Pgo4Result()
    res.Rcw = capi.ptr(sentinel, capi.c_double_p)
    res.tcw = capi.ptr(sentinel, capi.c_double_p)
    res.iterations, res.trials, res.status, res.envelope_tiles = -5, -6, 12345, -7
    before = bytes(C.string_at(C.addressof(res), C.sizeof(res)))
    rc = solver.lib.osh_pgo4_solve(solver.ctx, C.byref(prob), C.byref(res))
    assert rc == expect
    assert bytes(C.string_at(C.addressof(res), C.sizeof(res))) == before
    assert np.all(sentinel == 7.0)


def test_refusals_leave_the_result_untouched(solver):
    g = _graph(50)
    inv, uns = capi.OSH_ERR_INVALID, capi.OSH_ERR_UNSUPPORTED
    _refused(solver, g, inv, mutate=lambda p: setattr(p, "n_vertices", 0))
    bad = dataclasses.replace(g, edge_ij=g.edge_ij.copy())
    bad.edge_ij[3, 1] = len(g.fixed)
    _refused(solver, bad, inv)
    _refused(solver, g, inv, lambda_init=float("nan"))
    _refused(solver, g, inv, lambda_init=-1.0)
    # 4001 free vertices, then a graph under the vertex limit whose envelope is dense (every keyframe joined to the first)
    n = capi.OSH_PGO_MAX_VERTICES + 2
    eye = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    z = np.zeros((n, 3))
    fixed = np.zeros(n, bool)
    fixed[0] = True
    chain = np.c_[np.arange(1, n), np.arange(0, n - 1)].astype(np.int32)
    big = Pgo4Graph(eye, z, eye, z, eye, z, fixed, chain, np.broadcast_to(np.eye(3), (n - 1, 3, 3)).copy(), np.zeros((n - 1, 3)))
    _refused(solver, big, uns)
    m = capi.OSH_PGO_MAX_VERTICES
    star = np.c_[np.arange(2, m), np.ones(m - 2)].astype(np.int32)     # every keyframe joined to the first free one
    cap = Pgo4Graph(eye[:m], z[:m], eye[:m], z[:m], eye[:m], z[:m], np.r_[True, np.zeros(m - 1, bool)], np.r_[chain[:m - 1], star],
                    np.broadcast_to(np.eye(3), (2 * m - 3, 3, 3)).copy(), np.zeros((2 * m - 3, 3)))
    _refused(solver, cap, uns)


def test_4000_keyframes_complete(solver):
    g = _graph(4000, seed=9)
    assert int(np.count_nonzero(~g.fixed)) == capi.OSH_PGO_MAX_VERTICES - 1
    r = solver.solve4(g)
    assert r.iterations >= 1 and np.isfinite(r.chi2_final) and r.chi2_final < r.chi2_initial
    assert np.abs(r.Rwb[:, 2, :] - g.Rwb[:, 2, :]).max() <= 1e-12


# ---- through the reference signature (csrc/host/OptimizerEssentialGraph4DoF.cc) on stand-in maps ----
def _R(q):
    return sp._quat_to_R(np.asarray(q, np.float64))


@pytest.mark.parametrize("earlier", [False, True])
def test_reference_signature_write_back(solver, earlier):
    m = sp.make_inertial_loop(300, seed=4, earlier_loop=earlier, rp_noise=0.001, n_points=500)
    with sp.HostPgo4Map(m) as h:
        hg, ids = h.pack4()
        before_pose, before_pts = h.kf_poses(), h.mp_positions()
        r = solver.solve4(hg)                      # the device result for the host's own graph
        assert h.run4() == 0
        poses, pts = h.kf_poses(), h.mp_positions()
        assert h.change_index() == 1                                   # one IncreaseChangeIndex
        assert np.array_equal(h.normal_updates(), np.ones(len(m.mp_ref), int))   # one UpdateNormalAndDepth per point
    _, _, vScw = sp.pack_loop4(m, kf_pose=before_pose)
    index = {int(k): i for i, k in enumerate(m.kf_id)}
    for v, kid in enumerate(ids):
        i = index[int(kid)]
        # SE3d(Rcw, tcw) cast to float: the translation to the bit, the rotation to float precision
        assert np.array_equal(poses[i, 4:], r.tcw[v].astype(np.float32)), i
        assert np.abs(_R(poses[i, :4]) - r.Rcw[v]).max() <= 1e-6, i   # a float unit quaternion: a few float ulps
    # points: correctedSwr.map(Srw.map(P)) through the reference keyframe, Srw = vScw (the corrected Sim3 in CorrectedSim3)
    vert = {index[int(k)]: v for v, k in enumerate(ids)}
    quirk = 0
    for j, ref in enumerate(m.mp_ref):
        S = vScw[int(ref)]
        P = before_pts[j].astype(np.float64)
        p1 = S[7] * (_R(S[:4]) @ P) + S[4:7]
        v = vert[int(ref)]
        exp = r.Rcw[v].T @ (p1 - r.tcw[v])
        assert np.abs(pts[j] - exp).max() <= 2e-6 * max(1.0, np.abs(exp).max()), j
        if int(ref) in m.corrected:
            raw = sp.sim3_from_pose(before_pose[int(ref)])
            alt = r.Rcw[v].T @ ((_R(raw[:4]) @ P + raw[4:7]) - r.tcw[v])
            assert np.abs(alt - exp).max() > 1e-3     # the raw pose would have put the point elsewhere
            quirk += 1
    assert quirk > 0
    assert np.abs(poses - before_pose).max() > 1e-3


def test_reference_signature_4000_keyframes(solver):
    m = sp.make_inertial_loop(4000, seed=9, n_points=200)
    with sp.HostPgo4Map(m) as h:
        before = h.kf_poses()
        assert h.run4() == 0
        after = h.kf_poses()
        assert h.change_index() == 1
        assert np.array_equal(h.normal_updates(), np.ones(200, int))
    assert np.isfinite(after).all() and np.abs(after - before).max() > 1e-3
