"""The two dense LDL^T solvers of the reduced camera system on their own: csrc/ldlt_block.h (k_solve<NB, threads>, in LDS) and
csrc/big_solve.h (k_big_*, in global memory).

The systems come out of ``osh_lba_debug_trial``: S, b_s and x of one trial at a forced lambda, through whichever solver the upload
chose; ``osh_lba_get_solver`` says which, and every test asserts it.  The switches OSH_LBA_SOLVE_NB / _THREADS / _BIG and
OSH_LBA_DENSE_SOLVE (read at upload) pick the variant.

What every case asserts.  With x_ref the long-double refined solution of the very (S, b_s) the device exported
(solve_reference.py), eta the normwise backward error and eps the forward error:

    eta_dev <= M max(eta_ref, 2^-53)      eps_dev <= M max(eps_ref, 2^-53)

where (eta_ref, eps_ref) are those of the oracle's float64 no-pivot LDL^T (``ob.ldlt_solve``) on the same system (beyond 2000
unknowns, where that plain loop takes seconds, ``np.linalg.solve``).  test_solve_reference_cpu.py vets the windows: no zero pivot,
eps_ref < 1e-6, eta_ref <= 16 * 2^-53 (in fact eta_ref < 2^-53 everywhere, so the first bound is M 2^-53).

M = 64.  Measured on an MI355X, the largest ratios over every case of this file (MEASURED below): the backward error never exceeds
0.57 of the 2^-53 floor; the forward error reaches 13.3 times the oracle's for k_solve<12, *> (9 poses, long tracks, lambda 1e-3:
device 2.9e-13, oracle 2.2e-14 on a system of condition number 1.3e5, where the oracle itself reaches 1.7e-13 at the other lambda:
the scatter of two summation orders around kappa 2^-53, not a property of NB = 12), 5.0 for NB = 24, 4.7 for NB = 6 and 3.3 for
big_solve.h.  Four times the worst ratio is 53: the next power of two, 64, is M (no ratio is above 16).

Sizes of the LDS solver (optimisable poses; n = 6 per pose), each in two track styles (solve_cases.py), at lambda 1e-3 and 1e-8, with
NB in {24, 12, 6} x threads in {256, 512} x {envelope, OSH_LBA_DENSE_SOLVE=1}; envelope and dense must give the same bits of x:
    1 (n = 6: below every NB but 6), 2 (= NB 12), 3, 4 (= NB 24, one panel without padding), 5 (a full panel and a ragged one of 6),
    8 (two panels of 24), 9, 16 and 17 (around a multiple of 32 and of the 16-wide tile columns), 40 and 41 (ten NB = 24 panels, one more)
    116 and 235 with no override: the natural switches to NB = 12 and NB = 6
Sizes of the global-memory solver, forced with OSH_LBA_SOLVE_BIG=1:
    1 (a single ragged panel), 5 (below the panel width), 6 (first trailing block, 4 columns), 11, 16 (n = 96: the trailing block
    after the first panel is one 64-tile), 17, 32 and 33 (trailing blocks of 2 1/2 tiles: the upper-tile grid with a ragged edge), 43,
    100 (n = 600: k_big_back's eight-way unrolled loop needs more than 448 columns right of a panel)
    437, 438 and 439 with no override: the last LDS size of a single window, and the natural switch"""
import hashlib

import numpy as np
import pytest

import solve_cases as sc
import solve_reference as sr
from helpers import load_lba_fixture
from orb_slam3_study_kr_amd import lba
from test_gpu_lba import _check_result
from test_solve_plan_cpu import lds_bytes

pytestmark = pytest.mark.gpu

MEASURED_M = 64
# largest eta_dev / max(eta_ref, 2^-53) and eps_dev / max(eps_ref, 2^-53) seen per variant (one run on an MI355X)
MEASURED = {"big_solve": (0.562, 3.342), "k_solve<24,256>": (0.509, 4.976), "k_solve<24,512>": (0.509, 4.976),
            "k_solve<12,256>": (0.509, 13.264), "k_solve<12,512>": (0.509, 13.264), "k_solve<6,256>": (0.509, 4.747),
            "k_solve<6,512>": (0.509, 4.747)}
assert MEASURED_M == 64 >= 4 * max(max(v) for v in MEASURED.values())

KNOBS = dict(nb="OSH_LBA_SOLVE_NB", threads="OSH_LBA_SOLVE_THREADS", big="OSH_LBA_SOLVE_BIG", dense="OSH_LBA_DENSE_SOLVE",
             item="OSH_LBA_ITEM_MAX", chunk="OSH_LBA_CHUNK_EDGES")
# An upload cuts its Schur items and landmark chunks by the number of its windows (the sums then run in another order
# and the last bits of S depend on how many windows travel together).  The tests that compare a window of a batch with the same
# window alone pin both cuts to those of a single window, so that the two uploads hand the solver the same bits.
PIN = dict(item=24, chunk=256)
WORST = {}


@pytest.fixture(scope="module")
def solver(hip_lib):
    with lba.LbaSolver(0) as s:
        yield s


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for label in sorted(WORST):
        print(f"\nworst ratios {label:18s} eta {WORST[label][0]:7.3f}  eps {WORST[label][1]:7.3f}", end="")
    print()


def _upload(solver, mp, ws, **knobs):
    """Uploads `ws` with the given switches in the environment (they are read at upload) and returns what the upload chose."""
    for k, name in KNOBS.items():
        if knobs.get(k):
            mp.setenv(name, str(knobs[k]))
        else:
            mp.delenv(name, raising=False)
    try:
        solver.upload(ws)
    finally:
        for name in KNOBS.values():
            mp.delenv(name, raising=False)
    return solver.get_solver()


def _solve(solver, mp, ws, **knobs):
    got = _upload(solver, mp, ws, **knobs)
    solver.optimize()
    return got, solver.download()


def _label(got):
    return "big_solve" if got["big"] else f"k_solve<{got['nb']},{got['threads']}>"


def _reference(ob, cache, S, bs):
    """(x_ref, info, eta_ref, eps_ref) of the upper triangle of S and bs; the variants of one window export the same system."""
    key = hashlib.sha1((np.triu(S) + 0.0).tobytes() + (bs + 0.0).tobytes()).digest()      # (+ 0.0: one sign for the zeros)
    if key not in cache:
        x_ref, info = sr.solve_refined(S, bs)
        assert info["converged"], info["history"]
        if len(bs) <= 2000:
            ok, x = ob.ldlt_solve(info["A"], bs)
            assert ok
        else:
            x = np.linalg.solve(info["A"], bs)
        cache[key] = (x_ref, info) + sr.errors(info, x_ref, x)
    return cache[key]


def _check(ob, cache, got, S, bs, x, what):
    n = len(bs)
    assert np.isfinite(x).all()
    x_ref, info, eta_ref, eps_ref = _reference(ob, cache, S, bs)
    eta, eps = sr.errors(info, x_ref, x[:n])
    r_eta, r_eps = eta / max(eta_ref, sr.U53), eps / max(eps_ref, sr.U53)
    label = _label(got)
    print(f"{label:18s} {what}: eta {eta:.2e} (ref {eta_ref:.2e}, ratio {r_eta:.3f})  eps {eps:.2e} (ref {eps_ref:.2e}, ratio {r_eps:.3f})")
    w = WORST.setdefault(label, [0.0, 0.0])
    w[0], w[1] = max(w[0], r_eta), max(w[1], r_eps)
    assert r_eta <= MEASURED_M and r_eps <= MEASURED_M, (label, what, eta, eta_ref, eps, eps_ref)


@pytest.mark.parametrize("style", sc.STYLES)
@pytest.mark.parametrize("poses", sc.LDS_POSES)
def test_lds_solver_every_panel_width_thread_count_and_envelope(solver, ob, monkeypatch, poses, style):
    w = sc.window(poses, style)
    cache = {}
    for nb in (24, 12, 6):
        for threads in (256, 512):
            xs = {}
            for dense in (0, 1):
                got = _upload(solver, monkeypatch, [w], nb=nb, threads=threads, dense=dense)
                assert got == dict(big=False, nb=nb, threads=threads, lds_bytes=lds_bytes(nb, 6 * poses, threads))
                for lam in sc.LAMBDAS:
                    S, bs, x = solver.debug_trial(0, lam)
                    _check(ob, cache, got, S, bs, x, f"{poses} poses {style} {'dense' if dense else 'envelope'} lambda {lam:g}")
                    xs[dense, lam] = x
            for lam in sc.LAMBDAS:
                np.testing.assert_array_equal(xs[0, lam], xs[1, lam])      # the envelope skips exact zeros only: same bits
    assert len(cache) == len(sc.LAMBDAS)                                   # every variant was given the same two systems


@pytest.mark.parametrize("poses,n_points,nb", [(p, l, nb) for (p, l), nb in zip(sc.SWITCH_LDS, (12, 6))])
def test_lds_solver_natural_switch_points(solver, ob, monkeypatch, poses, n_points, nb):
    w = sc.switch_window(poses, n_points)
    got = _upload(solver, monkeypatch, [w])
    assert got == dict(big=False, nb=nb, threads=512, lds_bytes=lds_bytes(nb, 6 * poses, 512))
    assert lds_bytes(2 * nb, 6 * poses, 512) > 150 * 1024                  # the wider panel stopped fitting at exactly this size
    cache = {}
    for lam in sc.LAMBDAS:
        S, bs, x = solver.debug_trial(0, lam)
        _check(ob, cache, got, S, bs, x, f"{poses} poses, no override, lambda {lam:g}")


def test_window_whose_poses_do_not_fit_the_lds_of_backsub(solver, ob, monkeypatch):
    """Regression.  k_backsub kept x_p, the optimisable poses and the trial poses of all keyframes in LDS for every window of up to 512
    poses; from 394 optimisable poses (with two fixed ones) that is more than a block may have, and the launch failed with `invalid
    argument` (found by the 437-pose case below: no test window had more than 320).  Such a window now reads x_p and its poses
    from global memory.  One trial against the oracle, x_l included, at the tolerances of test_one_trial_schur_and_solution_match_oracle."""
    (poses, n_points), = sc.BACKSUB_GLOBAL
    w = sc.switch_window(poses, n_points)
    got = _upload(solver, monkeypatch, [w])
    assert got == dict(big=False, nb=6, threads=512, lds_bytes=lds_bytes(6, 6 * poses, 512))
    S, bs, x = solver.debug_trial(0, 1e-3)
    _check(ob, {}, got, S, bs, x, f"{poses} poses, no override, lambda 0.001")
    So, bso, xo = ob.lba_schur_step(w, 1e-3)
    iu = np.triu_indices(S.shape[0])
    np.testing.assert_allclose(S[iu], So[iu], rtol=1e-10, atol=1e-11 * np.abs(So).max())
    np.testing.assert_allclose(bs, bso, rtol=1e-10, atol=1e-11 * np.abs(bso).max())
    np.testing.assert_allclose(x, xo, rtol=1e-7, atol=1e-9 * np.abs(xo).max())


BIG = dict(big=True, nb=6, lds_bytes=0)


@pytest.mark.parametrize("style", sc.STYLES)
@pytest.mark.parametrize("poses", sc.BIG_POSES)
def test_global_memory_solver_forced(solver, ob, monkeypatch, poses, style):
    w = sc.window(poses, style)
    got = _upload(solver, monkeypatch, [w], big=1)
    assert got == dict(BIG, threads=512)
    cache = {}
    for lam in sc.LAMBDAS:
        S, bs, x = solver.debug_trial(0, lam)
        _check(ob, cache, got, S, bs, x, f"{poses} poses {style} lambda {lam:g}")


@pytest.mark.parametrize("poses,knobs,expect", [
    (437, {}, dict(big=False, nb=6, threads=512)),             # the last size a single window (512 threads) keeps in LDS
    (438, dict(threads=256), dict(big=False, nb=6, threads=256)),   # ... and the last of a 256-thread block
    (439, {}, dict(big=True, nb=6, threads=512)),
])
def test_natural_switch_to_the_global_memory_solver(solver, ob, monkeypatch, poses, knobs, expect):
    w = sc.switch_window(poses, dict(sc.SWITCH_BIG)[poses])
    got = _upload(solver, monkeypatch, [w], **knobs)
    assert {k: got[k] for k in expect} == expect
    assert got["lds_bytes"] == (0 if expect["big"] else lds_bytes(6, 6 * poses, expect["threads"]))
    cache = {}
    for lam in sc.LAMBDAS:
        S, bs, x = solver.debug_trial(0, lam)
        _check(ob, cache, got, S, bs, x, f"{poses} poses, {knobs or 'no override'}, lambda {lam:g}")
    if poses == 439:
        # 438 poses in one 512-thread block: one pose past its limit (upload only: the solve is the one of 439)
        assert _upload(solver, monkeypatch, [sc.switch_window(438, dict(sc.SWITCH_BIG)[438])]) == dict(BIG, threads=512)


def _trials(solver, ws, lam):
    return [solver.debug_trial(i, lam)[2] for i in range(len(ws))]


def test_global_memory_solver_batch_independence(solver, monkeypatch):
    """V, z and the fail flag are shared by the windows of a batch: 33, 6 and 17 poses in one upload, each x with the bits of its
    single-window upload."""
    ws = [sc.window(33, "short"), sc.window(6, "long"), sc.window(17, "short")]
    assert _upload(solver, monkeypatch, ws, big=1, **PIN) == dict(BIG, threads=512)
    batch = {lam: _trials(solver, ws, lam) for lam in sc.LAMBDAS}
    for i, w in enumerate(ws):
        assert _upload(solver, monkeypatch, [w], big=1, **PIN)["big"]
        for lam in sc.LAMBDAS:
            np.testing.assert_array_equal(batch[lam][i], solver.debug_trial(0, lam)[2])


@pytest.mark.parametrize("knobs", [dict(big=1), dict(nb=24), dict(nb=12), dict(nb=6), dict(nb=24, threads=256, dense=1)],
                         ids=["big", "nb24", "nb12", "nb6", "nb24-256-dense"])
def test_zero_pivot_in_the_middle_of_a_batch(solver, ob, monkeypatch, knobs):
    """A pose without any edge at lambda = 0: the pivot of unknown 42 is exactly zero (past the first panel of every variant).  The
    solver reports the failure as x_p = 0 (LinearSolverEigen::solve returning false); the windows before and after it in the batch
    are not touched, and the next trial of the same upload solves again (the flag is reset)."""
    mid = sc.zero_pivot_window()
    ws = [sc.window(8, "short"), mid, sc.window(5, "long")]
    got = _upload(solver, monkeypatch, ws, **knobs, **PIN)
    assert got["big"] == bool(knobs.get("big")) and (got["big"] or got["nb"] == knobs["nb"])
    S, bs, x = solver.debug_trial(1, 0.0)
    p, n = sc.ZERO_PIVOT_POSE, 6 * mid.n_free
    assert not sr.symmetric(S)[6 * p:6 * p + 6].any() and not bs[6 * p:6 * p + 6].any()
    assert not ob.ldlt_solve(sr.symmetric(S), bs)[0]                       # the oracle's factorisation fails on it too
    assert not x[:n].any()
    batch = _trials(solver, ws, 0.0)
    assert not batch[1][:n].any()
    cache = {}
    S, bs, x = solver.debug_trial(1, 1e-3)                                 # the same upload, now regular
    _check(ob, cache, got, S, bs, x, f"zero-pivot window at lambda 1e-3 after the failure ({knobs})")
    for i in (0, 2):
        assert _upload(solver, monkeypatch, [ws[i]], **knobs, **PIN)["big"] == got["big"]
        np.testing.assert_array_equal(batch[i], solver.debug_trial(0, 0.0)[2])


def test_edgeless_landmark_window_on_the_global_memory_path(solver, ob, monkeypatch):
    """The window of test_stop_flag_zero_iterations_and_empty_cases (a landmark seen by fixed keyframes only; its comment speaks of a
    zero pivot, but no pivot of it is zero: test_solve_reference_cpu.py) forced onto big_solve.h in the middle of a batch of three:
    its optimize() equals the oracle's and the LDS path's under _check_result, and its neighbours are as in uploads of their own."""
    w2 = sc.edgeless_landmark_window()
    ws = [sc.window(8, "short"), w2, sc.window(5, "long")]
    got, big = _solve(solver, monkeypatch, ws, big=1, **PIN)
    assert got["big"]
    got, lds = _solve(solver, monkeypatch, ws, **PIN)
    assert got == dict(big=False, nb=24, threads=512, lds_bytes=lds_bytes(24, 48, 512))
    _check_result(big[1], ob.lba_solve(w2), w2)
    _check_result(big[1], lds[1], w2)
    for i in (0, 2):
        _, alone = _solve(solver, monkeypatch, [ws[i]], big=1, **PIN)
        for k in ("pose_qt", "points", "chi2_trace", "lambda_trace", "trials_trace", "edge_chi2"):
            np.testing.assert_array_equal(getattr(big[i], k), getattr(alone[0], k))


@pytest.mark.parametrize("name", ["lba_tiny_stereo", "lba_tiny_reject_stereo"])
def test_full_lm_on_the_global_memory_path_matches_oracle(solver, ob, monkeypatch, name):
    w, _ = load_lba_fixture(name)
    got, res = _solve(solver, monkeypatch, [w], big=1)
    assert got["big"]
    _check_result(res[0], ob.lba_solve(w), w)


def test_global_memory_solver_history_independence(hip_lib, monkeypatch):
    """Forced big, the LDS path, forced big on a smaller window and on the first one again, all on one context: each result has the
    bits of a fresh context's (OSH_ZERO_NEW_BUFFERS=1 as in test_gpu_reuse.py, so the fresh side starts from zeros)."""
    monkeypatch.setenv("OSH_ZERO_NEW_BUFFERS", "1")
    steps = [(dict(big=1), sc.window(33, "short")), ({}, sc.window(41, "long")), (dict(big=1), sc.window(17, "long")),
             (dict(big=1), sc.window(33, "short"))]
    with lba.LbaSolver(0) as live:
        for knobs, w in steps:
            got, res = _solve(live, monkeypatch, [w], **knobs)
            x = live.debug_trial(0, 1e-3)[2]
            with lba.LbaSolver(0) as fresh:
                got_f, res_f = _solve(fresh, monkeypatch, [w], **knobs)
                x_f = fresh.debug_trial(0, 1e-3)[2]
            assert got == got_f and got["big"] == bool(knobs)
            np.testing.assert_array_equal(x, x_f)
            for k in ("pose_qt", "points", "chi2_trace", "lambda_trace", "trials_trace", "edge_chi2", "edge_depth_pos"):
                np.testing.assert_array_equal(getattr(res[0], k), getattr(res_f[0], k))
            assert res[0].iterations == res_f[0].iterations > 0
