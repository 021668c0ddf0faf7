"""k_schur_reduce (csrc/lba_reduce_solve.h): in a call of more than 8 windows 18 lanes reduce one block of S (or one rhs segment) of the
batch's block list, two entries per lane, 14 blocks per 256 threads; in a call of at most 8 windows 36 lanes, one entry per lane, 7 per
256 threads (k_schur_reduce_deep).  Which blocks share a wavefront and a thread block, and with which other window's blocks, depends on
where the window stands in the batch and on nothing else, so a window's S, b_s and its whole optimisation must not depend on the order
of the batch, bit for bit, nor on whether another window of the batch has already left optimize().
Small windows whose block counts P(P+1)/2 + P (2, 5, 35, 44, 54, 104) are multiples of neither 7 nor 14, with 50-800 landmarks, with
tracks of 2-4 observers (most blocks above the column envelope of S, blocks with one or no contribution) and of more than 8 (cross
items, many contributions per block: more than the eight a lane requests at once).  Two of the shapes are also checked against the CPU
oracle at the tolerances of tests/test_gpu_schur_cross.py."""
import dataclasses

import numpy as np
import pytest

from orb_slam3_study_kr_amd import lba, synth

pytestmark = pytest.mark.gpu

LAMBDA = 1e-3

# (n_free, n_fixed, landmarks, (shortest, longest) track)
SPECS = [
    (1, 2, 50, (2, 3)),
    (2, 2, 800, (2, 4)),
    (7, 2, 300, (3, 8)),       # oracle
    (8, 2, 120, (3, 10)),
    (9, 2, 500, (3, 11)),
    (13, 2, 800, (9, 15)),     # oracle: tracks of 9-13 optimisable observers
    (1, 3, 400, (2, 4)),
    (2, 1, 60, (2, 3)),
    (7, 2, 50, (2, 4)),
    (13, 2, 200, (2, 4)),      # poses more than three apart share no landmark: blocks above the envelope
    (9, 1, 700, (10, 10)),
    (8, 3, 640, (4, 11)),
]
ORACLE_SHAPES = (2, 5)   # indices into SPECS
# the two batch-size classes that launch different reduce kernels (results differ between the classes, never inside one)
BATCHES = {"batch": list(range(12)), "few": [2, 5, 0, 9, 3, 7]}


def _windows():
    return [synth.make_window(9100 + k, n_free=p, n_fixed=f, n_points=n, stereo=True, track_len=tl) for k, (p, f, n, tl) in enumerate(SPECS)]


def _solve(solver, ws):
    """S, b_s of one trial and the result of optimize() of every window of the batch ``ws``."""
    solver.upload(ws)
    trials = [solver.debug_trial(k, LAMBDA)[:2] for k in range(len(ws))]
    solver.optimize()
    return [(S, bs, r) for (S, bs), r in zip(trials, solver.download())]


def _assert_same(a, b, with_S=True):
    (Sa, bsa, ra), (Sb, bsb, rb) = a, b
    if with_S:
        iu = np.triu_indices(Sa.shape[0])
        np.testing.assert_array_equal(Sa[iu], Sb[iu])
        np.testing.assert_array_equal(bsa, bsb)
    assert (ra.iterations, ra.trials) == (rb.iterations, rb.trials)
    np.testing.assert_array_equal(ra.trials_trace, rb.trials_trace)
    np.testing.assert_array_equal(ra.chi2_trace, rb.chi2_trace)
    np.testing.assert_array_equal(ra.lambda_trace, rb.lambda_trace)
    np.testing.assert_array_equal(ra.pose_qt, rb.pose_qt)
    np.testing.assert_array_equal(ra.points, rb.points)


@pytest.fixture(scope="module")
def solver(hip_lib):
    with lba.LbaSolver(0) as s:
        yield s


@pytest.fixture(scope="module")
def windows():
    return _windows()


@pytest.fixture(scope="module")
def base(solver, windows):
    """name -> results of the batch in its own order (computed once, read by every test)"""
    return {name: _solve(solver, [windows[k] for k in idx]) for name, idx in BATCHES.items()}


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_the_windows_are_what_they_are_there_for(windows, base, name):
    ws = [windows[k] for k in BATCHES[name]]
    assert {w.n_free for w in windows} == {1, 2, 7, 8, 9, 13} and all(50 <= n <= 800 for _, _, n, _ in SPECS) and all(w.n_points > 0 for w in windows)
    free_obs = lambda w: np.bincount(w.edge_point[w.edge_pose < w.n_free], minlength=w.n_points)
    assert free_obs(windows[5]).max() > 8 and free_obs(windows[10]).max() > 8 and free_obs(windows[1]).max() <= 4
    # blocks above the envelope exist (and stay zero), every window iterates
    S9 = base["batch"][9][0]
    assert not S9[:6, -6:].any() and S9[:6, :6].any()
    assert all(r.iterations > 0 for _, _, r in base[name])
    assert len(ws) > 8 if name == "batch" else 3 <= len(ws) <= 8


@pytest.mark.parametrize("order", ["reversed", "rotated"])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_results_do_not_depend_on_the_position_in_the_batch(solver, windows, base, name, order):
    idx = BATCHES[name]
    n = len(idx)
    perm = list(range(n))[::-1] if order == "reversed" else [(k + 5) % n for k in range(n)]
    got = _solve(solver, [windows[idx[k]] for k in perm])
    for pos, k in enumerate(perm):
        _assert_same(got[pos], base[name][k])


@pytest.mark.parametrize("how", ["max_iterations", "stop_flag"])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_a_window_that_stopped_does_not_move_the_others(solver, windows, base, name, how):
    idx = BATCHES[name]
    at = 1   # neither the first nor the last window of the batch
    ws = [windows[k] for k in idx]
    if how == "max_iterations":
        ws[at] = dataclasses.replace(ws[at], max_iterations=1)
    else:
        ws[at] = dataclasses.replace(ws[at], stop_flag=np.ones(1, dtype=np.uint8))
    got = _solve(solver, ws)
    assert got[at][2].iterations <= 1 < base[name][at][2].iterations
    if how == "stop_flag":
        assert got[at][2].iterations == 0
    for k in range(len(ws)):
        if k != at:
            # debug_trial reduces every window (it runs before any controller decision), optimize() only the active ones
            _assert_same(got[k], base[name][k])


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_one_trial_against_the_oracle(windows, base, shape):
    from oracle import binding as ob
    S, bs, _ = base["batch"][shape]
    So, bso, _ = ob.lba_schur_step(windows[shape], LAMBDA)
    iu = np.triu_indices(S.shape[0])
    np.testing.assert_allclose(S[iu], So[iu], rtol=1e-10, atol=1e-11 * np.abs(So).max())
    np.testing.assert_allclose(bs, bso, rtol=1e-10, atol=1e-11 * np.abs(bso).max())
