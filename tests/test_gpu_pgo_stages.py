"""Stage-by-stage GPU checks of the Sim3 pose graph (osh_pgo_*, csrc/pgo_device.hip) against an extended-precision reference.

Each test isolates one stage so that a failure names it: the error and numeric Jacobians with assembly (osh_pgo_linearize
against pgo_numpy in np.longdouble), the envelope LDL^T and the step (one accepted trial against an iteratively refined
long-double solve of the device's own H and b), the Levenberg-Marquardt controller (trial sequences of pgo_numpy.optimize),
and the C-ABI's refusals and size limits.  Graphs are built directly (pgo_cases.py) in the shapes where the envelope's
32-row tiles, the active lists and the Sim3 branches go wrong."""
import ctypes as C

import numpy as np
import pytest

import pgo_cases as pc
import pgo_numpy as pn
from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_pgo as sp
from orb_slam3_study_kr_amd.pgo import PgoGraph, PgoSolver

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def solver():
    pn.require_extended()
    with PgoSolver(0) as s:
        yield s


def _dev(g):
    return PgoGraph(np.asarray(g.estimate, np.float64), np.asarray(g.fixed, bool), np.asarray(g.fix_scale, bool),
                    np.asarray(g.edge_ij, np.int32).reshape(-1, 2), np.asarray(g.measurement, np.float64).reshape(-1, 8))


def _np(g):
    return pn.PgoGraph(g.estimate, g.fixed, g.fix_scale, g.edge_ij, g.measurement)


# ---- a. the Sim3 branches through error, Jacobians and assembly ----

def _branch_graph(u, side, fix_scale, seed):
    rng = np.random.default_rng(seed)
    S = pc.random_sim3(rng, 3, t_scale=2.0)
    fixed = np.array([True, False, True])       # vertex 2: a fixed vertex no edge touches
    fs = np.array([False, fix_scale, False])
    i, j = (1, 0) if side == 0 else (0, 1)
    meas = pc.measurement_for(u, S[i], S[j])[None]
    return pn.PgoGraph(S, fixed, fs, np.array([[i, j]], np.int32), meas)


def test_sim3_branch_table(solver):
    cases = []
    for k, (name, u) in enumerate(pc.branch_table()):
        for side in (0, 1):
            for fs in (False, True):
                cases.append((name, float(f"{np.linalg.norm(u[:3]):.3g}"), f"{name}/side{side}/fs{int(fs)}", _branch_graph(u, side, fs, 100 + k)))
    rows = []
    for _, th, name, g in cases:
        chi2, H, b = solver.linearize(_dev(g))
        c_ld, H_ld, b_ld = pn.linearize(g, g.estimate, LD)
        c_64, H_64, b_64 = pn.linearize(g, g.estimate)
        # 1e-13, or 2.5x numpy's own distance where g2o's formula amplifies rounding (the 1 / sigma^2 of the small-angle A)
        tol = max(1e-13, 2.5 * abs(c_64 - float(c_ld)) / float(c_ld))
        assert abs(chi2 - float(c_ld)) <= tol * float(c_ld), (name, chi2, float(c_ld), c_64)
        rows.append((th, name, pc.block_errors(H, H_ld, 1).max(), pc.block_errors(H_64, H_ld, 1).max(),
                     pc.block_errors(b, b_ld, 1).max(), pc.block_errors(b_64, b_ld, 1).max()))
    # bounds per rotation angle: the float64 central difference of log() is as good as ~3e-6 up to theta = 2, but near pi
    # (theta = 3: 1 / sin(theta) ~ 7) numpy's own error reaches ~9e-5, so there only the relative bound applies
    print(f"\nbranch table, {len(rows)} cases: max per-block error vs long double")
    for th in sorted({r[0] for r in rows}):
        grp = [r for r in rows if r[0] == th]
        np_h, np_b = max(r[3] for r in grp), max(r[5] for r in grp)
        dv_h, dv_b = max(r[2] for r in grp), max(r[4] for r in grp)
        print(f"  theta {th:g}: H device {dv_h:.2e} numpy {np_h:.2e} ratio {dv_h / np_h:.2f} | b device {dv_b:.2e} numpy {np_b:.2e} "
              f"ratio {dv_b / np_b:.2f}")
        cap = 5e-6 if th <= 2.0 else 2e-4
        for _, name, dh, _, db, _ in grp:
            assert dh <= min(2.5 * np_h, cap), (name, dh, np_h)
            assert db <= min(2.5 * np_b, cap), (name, db, np_b)


def test_sim3_branch_thresholds_error_only(solver):
    # within ~1e-8 of a branch threshold g2o's own central difference is discontinuous: only the error (chi2) is compared
    for k, (name, u) in enumerate(pc.near_threshold_table()):
        for side in (0, 1):
            g = _branch_graph(u, side, False, 200 + k)
            chi2, _, _ = solver.linearize(_dev(g))
            c_ld = float(pn.linearize(g, g.estimate, LD)[0])
            assert abs(chi2 - c_ld) <= 1e-13 * c_ld, (name, side, chi2, c_ld)
            res = solver.solve(_dev(g), iterations=1)
            assert abs(res.chi2_initial - c_ld) <= 1e-13 * c_ld, name


# ---- b. the Jacobian-noise explanation of DESIGN.md section 9 ----

@pytest.mark.parametrize("n,mono", [(50, True), (50, False), (300, True), (300, False)])
def test_jacobian_noise_no_worse_than_float64_reference(solver, n, mono):
    m = sp.make_map(n, seed=11, mono=mono)
    g, _, _ = sp.pack_loop(m)
    G = _np(g)
    _, H, b = solver.linearize(g)
    _, H_64, b_64 = pn.linearize(G, G.estimate)
    _, H_ld, b_ld = pn.linearize(G, G.estimate, LD)
    nf = H.shape[0] // 7
    dh, nh = pc.block_errors(H, H_ld, nf), pc.block_errors(H_64, H_ld, nf)
    db, nb = pc.block_errors(b, b_ld, nf), pc.block_errors(b_64, b_ld, nf)
    print(f"\nn={n} mono={mono}: per-block relative error vs long double  H device max {dh.max():.2e} median {np.median(dh):.2e}"
          f" | numpy max {nh.max():.2e} median {np.median(nh):.2e};  b device max {db.max():.2e} median {np.median(db):.2e}"
          f" | numpy max {nb.max():.2e} median {np.median(nb):.2e}")
    assert dh.max() <= 3 * nh.max() and np.median(dh) <= 3 * np.median(nh)
    assert db.max() <= 3 * nb.max() and np.median(db) <= 3 * np.median(nb)


# ---- c. the linear solve and the step, on the device's own H and b ----

def _chain(nf):
    return [(a, a + 1) for a in range(nf - 1)]


def _with_anchor(nf, edges, fixed_free=(), fix_scale=False, seed=0, extra_fixed_edges=()):
    """nf free vertices 0..nf-1 (free index = array index) plus one fixed anchor nf joined to vertex 0; fixed_free lists
    further vertices among 0..nf-1 to fix (they stay in the array, so later free indices shift down)."""
    e = list(edges) + [(nf, 0)] + list(extra_fixed_edges)
    return pc.make_graph(nf + 1, e, fixed=(nf,) + tuple(fixed_free), fix_scale=fix_scale, seed=seed)


def _solve_shapes():
    S = {}
    for nf in (1, 4, 5, 9, 32, 33, 37, 64, 69, 512):
        S[f"chain{nf}"] = _with_anchor(nf, _chain(nf), seed=nf)
        if nf > 2:
            S[f"chain{nf}+loop"] = _with_anchor(nf, _chain(nf) + [(nf - 1, 0)], seed=1000 + nf)
    # newest vertex's first non-zero on a tile's first row (vertex 32: row 224 = 7 * 32) and one row before (vertex 9: row 63)
    S["loops_tile_edge"] = _with_anchor(69, _chain(69) + [(60, 32), (68, 9)], seed=3)
    S["loops_three"] = _with_anchor(69, _chain(69) + [(60, 32), (68, 9), (45, 0)], seed=4)
    S["hub_first"] = pc.make_graph(40, [(0, v) for v in range(1, 40)] + _chain(40)[5:], fixed=(20,), seed=5)
    S["hub_last"] = pc.make_graph(40, [(v, 39) for v in range(0, 39)] + _chain(39), fixed=(0,), seed=6)
    rng = np.random.default_rng(7)
    dense_edges = [(a, b) for a in range(40) for b in range(a + 1, 40) if rng.random() < 0.3] + _chain(40)
    S["random30"] = _with_anchor(40, dense_edges, seed=7)
    for tag, fx in (("first", (0,)), ("middle", (10,)), ("last", (19,)), ("several", (0, 7, 13, 19))):
        S[f"fixed_{tag}"] = pc.make_graph(20, _chain(20) + [(19, 2)], fixed=fx, seed=8)
    S["isolated_free"] = pc.make_graph(11, _chain(5) + [(a, a + 1) for a in range(6, 10)] + [(4, 6)], fixed=(0,), seed=9)
    S["fixed_fixed_edge"] = pc.make_graph(12, _chain(12) + [(1, 0), (11, 1)], fixed=(0, 1), seed=10)
    S["both_directions"] = pc.make_graph(12, _chain(12) + [(4, 3), (3, 4), (9, 2), (2, 9)], fixed=(0,), seed=11)
    fs = np.arange(40) % 3 == 1
    S["mixed_fix_scale"] = pc.make_graph(40, _chain(40) + [(39, 1), (25, 3)], fixed=(0,), fix_scale=fs, seed=12)
    S["rotate_130deg"] = _big_rotation()
    return S


def _big_rotation():
    # one free vertex whose measurement puts it 130 degrees from its estimate: the step's exp() lands in R_to_quat's
    # trace <= 0 branch (tr R = 1 + 2 cos 130deg < 0) in k_pgo_step
    rng = np.random.default_rng(13)
    S = pc.random_sim3(rng, 2, t_scale=1.0)
    ax = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    u = np.concatenate([ax * np.deg2rad(130.0), [0.2, -0.1, 0.3], [0.1]])
    meas = pc.measurement_for(u, S[0], S[1])[None]
    return pn.PgoGraph(S, np.array([True, False]), np.array([False, False]), np.array([[0, 1]], np.int32), meas)


SHAPES = _solve_shapes()


@pytest.mark.parametrize("name", list(SHAPES))
def test_linear_solve_and_step(solver, name):
    g = SHAPES[name]
    _, H, b = solver.linearize(_dev(g))
    nf = H.shape[0] // 7
    free = np.flatnonzero(~g.fixed)
    lam = 1e-3 * max(float(np.abs(np.diag(H)).max()), 1e-300)
    A = H + lam * np.eye(len(b))
    ev = np.linalg.eigvalsh(A)
    kappa = float(ev.max() / ev.min())
    x = pn.solve_ld(A, b)
    exp_est = pn.oplus(np.asarray(g.estimate[free], LD), x.reshape(nf, 7), g.fix_scale[free], LD)
    xinf = float(np.abs(x).max())
    estinf = float(np.abs(g.estimate).max())
    # the solve's error bound, carried through exp(x) * S (a step error dx moves S by ~(1 + |S|) dx), plus the rounding of
    # the float64 step itself
    tol = 20 * U53 * kappa * xinf * (1 + estinf) + 1e-15 * max(1.0, estinf)
    stats = pc.envelope_stats(g)
    for dense in (False, True):
        res = solver.solve(_dev(g), iterations=1, lambda_init=lam, dense=dense)
        assert (res.iterations, res.trials) == (1, 1), (name, dense)
        err = float(np.abs(np.asarray(res.estimate[free], LD) - exp_est).max())
        print(f"\n{name} {'dense' if dense else 'envelope'}: nf={nf} kappa={kappa:.2e} |x|={xinf:.2e} step err {err:.2e} "
              f"ratio {err / tol:.3f}")
        assert err <= tol, (name, dense, err, tol)
        assert res.estimate[g.fixed].tobytes() == g.estimate[g.fixed].tobytes()
        exp_stats = pc.envelope_stats(g, dense=dense)
        assert (res.envelope_tiles, res.envelope_entries, res.tall_columns) == exp_stats, (name, dense)
        if not dense:
            assert exp_stats == stats
    if name == "isolated_free":
        iso = 5
        assert not np.any(H[7 * (iso - 1):7 * iso])     # free index 4 (vertex 0 is fixed): no edge, no row
        for dense in (False, True):
            res = solver.solve(_dev(g), iterations=1, lambda_init=lam, dense=dense)
            assert res.estimate[iso].tobytes() == g.estimate[iso].tobytes()
    if name == "rotate_130deg":
        R = pn.quat_to_R(np.asarray(exp_est[0], np.float64))
        step_R = pn.quat_to_R(pn.sim3_exp(np.asarray(x[:7], np.float64))[:4])
        assert np.trace(step_R) < 0, np.trace(step_R)
        assert np.isfinite(R).all()


# ---- d. the Levenberg-Marquardt controller ----

def _consistent_graph(n=12):
    # translations on a small integer grid, unit scale and rotation: every error is exactly zero, chi2 == 0
    rng = np.random.default_rng(21)
    t = rng.integers(-4, 5, size=(n, 3)).astype(np.float64)
    est = np.zeros((n, 8))
    est[:, 3] = 1.0
    est[:, 4:7] = t
    est[:, 7] = 1.0
    eij = np.array(_chain(n) + [(n - 1, 0), (5, 2)], np.int32)
    meas = np.zeros((len(eij), 8))
    meas[:, 3] = 1.0
    meas[:, 7] = 1.0
    meas[:, 4:7] = t[eij[:, 1]] - t[eij[:, 0]]
    fx = np.zeros(n, bool)
    fx[0] = True
    return pn.PgoGraph(est, fx, np.zeros(n, bool), eij, meas)


def _controller_cases():
    # (graph, lambda_init, iterations); every trial's rho is far from 0 (|rho| > 0.1, pgo_numpy.optimize's trace), so no
    # accept / reject decision depends on rounding
    loop = lambda seed, drift: pc.make_graph(30, _chain(30) + [(29, 0), (20, 5)], fixed=(0,), seed=seed, noise=1e-2, drift=drift)
    return {
        "consistent": (_consistent_graph(), 1e-16, 20),
        # accepted steps with lambda shrinking from 1e6 (rho 0.92 .. 8.6, one rejection at rho -3.3)
        "large_lambda": (loop(22, 0.1), 1e6, 12),
        # a strongly non-linear first step: nine rejections at rho -2.1, the tenth trial accepted, the maxTrials stop
        "rejected_first": (loop(23, 0.8), 1e-16, 20),
        # three accepted trials (rho 0.54, 0.64, 0.73) that each lower chi2 by ~4e-5 of itself: the three-small-decreases stop
        "three_small": (loop(22, 0.1), 1e7, 20),
    }


CONTROLLER = _controller_cases()


@pytest.mark.parametrize("name", list(CONTROLLER))
def test_lm_controller_paths(solver, name):
    g, lam, its = CONTROLLER[name]
    trace = []
    ref = pn.optimize(g, iterations=its, lambda_init=lam, trace=trace)
    if name != "consistent":
        assert min(abs(t[1]) for t in trace) > 0.1, trace
    res = solver.solve(_dev(g), iterations=its, lambda_init=lam)
    print(f"\n{name}: it {res.iterations}/{ref.iterations} tr {res.trials}/{ref.trials} chi2 {res.chi2_initial:.6g} -> "
          f"{res.chi2_final:.9g} / {ref.chi2_final:.9g}")
    assert (res.iterations, res.trials) == (ref.iterations, ref.trials)
    # chi2_final within 1e-9, or within the distance by which the float64 rounding of the numeric Jacobians alone moves it:
    # the same run with the Jacobians taken in long double (the device's Jacobians are as far from long double as numpy's,
    # test_jacobian_noise_no_worse_than_float64_reference; a step far from the minimum passes that on to first order)
    ref_ld = pn.optimize(g, iterations=its, lambda_init=lam, jacobian_dtype=LD)
    assert (ref_ld.iterations, ref_ld.trials) == (ref.iterations, ref.trials)
    spread = abs(ref_ld.chi2_final - ref.chi2_final)
    diff = abs(res.chi2_final - ref.chi2_final)
    print(f"  chi2_final: device - numpy {diff:.3g}, numpy long-double Jacobians - numpy {spread:.3g}")
    assert diff <= max(1e-9 * ref.chi2_final, spread), (diff, spread)
    if name == "consistent":
        assert ref.chi2_initial == 0.0 and res.chi2_initial == 0.0
        assert (res.iterations, res.trials) == (1, 1)
        assert res.estimate.tobytes() == g.estimate.tobytes()
    elif name == "large_lambda":
        assert res.iterations == its and res.chi2_final < 0.1 * res.chi2_initial
        assert [t[2] for t in trace if t[3]][-1] < 1e-3 * lam
    elif name == "rejected_first":
        assert res.trials > res.iterations and not trace[0][3]
    elif name == "three_small":
        assert res.iterations == res.trials == 3 and all(t[3] for t in trace)


# ---- e. the C-ABI's refusals and limits ----

SENTINEL = 1234.5


def _raw_solve(solver, g, iterations=1, lambda_init=1e-16, solve_mode=capi.OSH_PGO_SOLVE_ENVELOPE):
    gd = _dev(g) if not isinstance(g, PgoGraph) else g
    prob = gd.as_struct(iterations, lambda_init, solve_mode)
    out = np.full((len(gd.estimate), 8), SENTINEL)
    res = capi.PgoResult()
    res.estimate = capi.ptr(out, capi.c_double_p)
    rc = solver.lib.osh_pgo_solve(solver.ctx, C.byref(prob), C.byref(res))
    return rc, res, out


def _refused(solver, g, code, **kw):
    rc, _, out = _raw_solve(solver, g, **kw)
    assert rc == code, (rc, capi.last_error(solver.lib))
    assert capi.last_error(solver.lib)
    assert np.all(out == SENTINEL)


def test_empty_graphs_are_solved_unchanged(solver):
    g = pc.make_graph(5, _chain(5), fixed=(0, 1, 2, 3, 4), seed=30)        # nf = 0
    rc, res, out = _raw_solve(solver, g, iterations=5)
    assert rc == capi.OSH_OK and out.tobytes() == g.estimate.tobytes()
    g = pc.make_graph(5, [], fixed=(0,), seed=31)                          # E = 0
    rc, res, out = _raw_solve(solver, g, iterations=5)
    assert rc == capi.OSH_OK and out.tobytes() == g.estimate.tobytes() and res.chi2_final == 0.0


@pytest.mark.parametrize("edge", [(2, 2), (1, 7), (-1, 2)])
def test_bad_edge_is_refused(solver, edge):
    g = pc.make_graph(5, _chain(5), fixed=(0,), seed=32)
    g.edge_ij[1] = edge
    _refused(solver, g, capi.OSH_ERR_INVALID)


@pytest.mark.parametrize("lam", [0.0, -1.0, float("nan")])
def test_bad_lambda_is_refused(solver, lam):
    _refused(solver, pc.make_graph(5, _chain(5), fixed=(0,), seed=33), capi.OSH_ERR_INVALID, lambda_init=lam)


def test_unknown_solve_mode_is_refused(solver):
    _refused(solver, pc.make_graph(5, _chain(5), fixed=(0,), seed=34), capi.OSH_ERR_INVALID, solve_mode=2)


def _big(nf, edges):
    # cheap to build: identity-rotation vertices along a line, measurements equal to the relative poses
    est = np.zeros((nf + 1, 8))
    est[:, 3] = 1.0
    est[:, 4] = np.arange(nf + 1) * 0.1
    est[:, 7] = 1.0
    eij = np.array(list(edges) + [(nf, 0)], np.int32)
    meas = np.zeros((len(eij), 8))
    meas[:, 3] = 1.0
    meas[:, 7] = 1.0
    meas[:, 4] = est[eij[:, 1], 4] - est[eij[:, 0], 4] + 1e-3
    fx = np.zeros(nf + 1, bool)
    fx[nf] = True
    return PgoGraph(est, fx, np.zeros(nf + 1, bool), eij, meas)


def test_vertex_limit_at_the_c_abi(solver):
    rc, res, _ = _raw_solve(solver, _big(4000, _chain(4000)))
    assert rc == capi.OSH_OK and (res.iterations, res.trials) == (1, 1)
    _refused(solver, _big(4001, _chain(4001)), capi.OSH_ERR_UNSUPPORTED)


def test_envelope_tile_cap(solver):
    hub = lambda nf: _big(nf, [(0, v) for v in range(1, nf)])
    g = hub(1650)
    assert pc.envelope_stats(g)[0] == 65341 and pc.envelope_stats(hub(1651))[0] == 65703
    rc, res, _ = _raw_solve(solver, g)
    assert rc == capi.OSH_OK and res.envelope_tiles == 65341 and (res.iterations, res.trials) == (1, 1)
    _refused(solver, hub(1651), capi.OSH_ERR_UNSUPPORTED)
    rc, res, _ = _raw_solve(solver, _big(1650, _chain(1650)), solve_mode=capi.OSH_PGO_SOLVE_DENSE)
    assert rc == capi.OSH_OK and res.envelope_tiles == 65341
    _refused(solver, _big(1651, _chain(1651)), capi.OSH_ERR_UNSUPPORTED, solve_mode=capi.OSH_PGO_SOLVE_DENSE)


def test_linearize_size_limit(solver):
    chi2, H, b = solver.linearize(_big(512, _chain(512)))
    assert H.shape == (3584, 3584) and chi2 > 0
    g = _big(513, _chain(513))
    prob = g.as_struct()
    N = 7 * 513
    H = np.full((N, N), SENTINEL)
    b = np.full(N, SENTINEL)
    c2 = np.full(1, SENTINEL)
    rc = solver.lib.osh_pgo_linearize(solver.ctx, C.byref(prob), capi.ptr(H, capi.c_double_p), capi.ptr(b, capi.c_double_p),
                                      capi.ptr(c2, capi.c_double_p))
    assert rc == capi.OSH_ERR_UNSUPPORTED and capi.last_error(solver.lib)
    assert np.all(H == SENTINEL) and np.all(b == SENTINEL) and c2[0] == SENTINEL
