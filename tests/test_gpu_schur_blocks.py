"""Symmetric Schur items from 4 x 4 blocks (csrc/lba_schur_items.h:k_schur_fused<true, false, true>): the diagonal tiles and the ragged
last tile column of a symmetric pinhole item are formed with v_mfma_f64_4x4x4_4b_f64 over the k sequence of the whole tiles, so every
entry of S keeps its bits.  Nine small windows of 1 ... 8 and 12 optimisable keyframes, each uploaded alone, which together hold
symmetric items of every number of row poses, of one to three chunks (8 x 8 lanes; one and two in the 12 x 5 and 16 x 4 mappings, whose
items of at most 24 landmarks have no more; the batch below cuts at 64) and with partial last chunks in every mapping
(asserted through the host-only plan export, so that a change of synth cannot hollow the test out): S, b_s of one trial against the CPU
oracle at the bounds of tests/test_gpu_schur_cross.py; S, b_s and the whole optimisation bit for bit against the whole-tile path
(OSH_LBA_SCHUR_TILES=1, read at upload) in a fresh context; and in one batch of the nine, each window's result equal to its result
alone, as tests/test_gpu_schur_reduce.py checks."""
import numpy as np
import pytest

from orb_slam3_study_kr_amd import lba, synth

pytestmark = pytest.mark.gpu

LAMBDA = 1e-3
NS = [1, 2, 3, 4, 5, 6, 7, 8, 12]
LANES = {nx: 16 if nx <= 4 else (12 if nx == 5 else 8) for nx in range(1, 9)}   # landmarks per chunk of an item of nx row poses


def _window(n):
    return synth.make_window(40 + n, n_free=n, n_fixed=2, n_points=60, stereo=True, track_len=(2, n + 2))


def _run(solver, ws):
    """S, b_s of one trial and the result of optimize() of every window of the batch ``ws``."""
    solver.upload(ws)
    trials = [solver.debug_trial(k, LAMBDA)[:2] for k in range(len(ws))]
    solver.optimize()
    return [(S, bs, r) for (S, bs), r in zip(trials, solver.download())]


def _assert_same(a, b):
    (Sa, bsa, ra), (Sb, bsb, rb) = a, b
    iu = np.triu_indices(Sa.shape[0])
    np.testing.assert_array_equal(Sa[iu], Sb[iu])
    np.testing.assert_array_equal(bsa, bsb)
    assert (ra.iterations, ra.trials) == (rb.iterations, rb.trials) and ra.iterations > 0
    np.testing.assert_array_equal(ra.trials_trace, rb.trials_trace)
    np.testing.assert_array_equal(ra.chi2_trace, rb.chi2_trace)
    np.testing.assert_array_equal(ra.lambda_trace, rb.lambda_trace)
    np.testing.assert_array_equal(ra.pose_qt, rb.pose_qt)
    np.testing.assert_array_equal(ra.points, rb.points)


@pytest.fixture(scope="module")
def windows():
    return {n: _window(n) for n in NS}


@pytest.fixture(scope="module")
def alone(hip_lib, windows):
    """n -> (S, b_s, result) of the window uploaded alone, blocks (computed once, read by every test)"""
    with lba.LbaSolver(0) as s:
        return {n: _run(s, [windows[n]])[0] for n in NS}


@pytest.fixture(scope="module")
def alone_tiles(hip_lib, windows):
    """the same with whole tiles, in a context of its own"""
    mp = pytest.MonkeyPatch()
    mp.setenv("OSH_LBA_SCHUR_TILES", "1")
    try:
        with lba.LbaSolver(0) as s:
            return {n: _run(s, [windows[n]])[0] for n in NS}
    finally:
        mp.undo()


def test_the_windows_hold_every_item_shape(windows):
    shapes = {}
    for n in NS:
        for k, v in lba.schur_plan_shapes(windows[n])[0].items():
            shapes[k] = shapes.get(k, 0) + v
    sym = [(nx, lm) for (s, nx, ny, lm) in shapes if s == 1]
    assert {nx for nx, _ in sym} == set(range(1, 9))
    chunks = lambda nx, lm: -(-lm // LANES[nx])
    for lanes in (16, 12, 8):
        mine = [(nx, lm) for nx, lm in sym if LANES[nx] == lanes]
        assert {chunks(nx, lm) for nx, lm in mine} >= ({1, 2, 3} if lanes == 8 else {1, 2}), (lanes, sorted(mine))
        assert any(lm % lanes for _, lm in mine), (lanes, sorted(mine))            # a partial last chunk
    assert {1, 2, 3} <= {chunks(nx, lm) for nx, lm in sym}
    assert {lm for _, lm in sym} >= {24, 22, 16, 11, 5, 3, 1}
    assert {(nx, ny) for (s, nx, ny, _) in shapes if s == 0} >= {(8, 4), (8, 2), (8, 1)}
    assert all(s == 1 for n in NS[:8] for (s, *_) in lba.schur_plan_shapes(windows[n])[0])


@pytest.mark.parametrize("n", NS)
def test_one_trial_against_the_oracle(windows, alone, n):
    from oracle import binding as ob
    S, bs, _ = alone[n]
    So, bso, _ = ob.lba_schur_step(windows[n], LAMBDA)
    iu = np.triu_indices(S.shape[0])
    np.testing.assert_allclose(S[iu], So[iu], rtol=1e-10, atol=1e-11 * np.abs(So).max())
    np.testing.assert_allclose(bs, bso, rtol=1e-10, atol=1e-11 * np.abs(bso).max())


@pytest.mark.parametrize("n", NS)
def test_the_same_bits_as_whole_tiles(alone, alone_tiles, n):
    _assert_same(alone[n], alone_tiles[n])


def test_a_window_in_a_batch_equals_the_window_alone(hip_lib, windows):
    # A call of nine windows cuts its items at 64 landmarks and its landmark-major chunks at 1024 edges, a call of one at 24 and 256
    # (schur_plan.h:item_max_lm, lba_pack.h:chunk_max_edges): other partial sums.  The windows alone are given the cuts of the batch;
    # what is left to differ is where a window stands in the batch, which reduce kernel sums it, and the items of up to 60 landmarks.
    mp = pytest.MonkeyPatch()
    mp.setenv("OSH_LBA_ITEM_MAX", "64")
    mp.setenv("OSH_LBA_CHUNK_EDGES", "1024")
    try:
        with lba.LbaSolver(0) as s:
            got = _run(s, [windows[n] for n in NS])
            one = [_run(s, [windows[n]])[0] for n in NS]
        mp.setenv("OSH_LBA_SCHUR_TILES", "1")
        with lba.LbaSolver(0) as s:
            ref = _run(s, [windows[n] for n in NS])
    finally:
        mp.undo()
    for k in range(len(NS)):
        _assert_same(got[k], one[k])
        _assert_same(got[k], ref[k])
