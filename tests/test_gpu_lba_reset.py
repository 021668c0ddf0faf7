"""What osh_lba_optimize does before its first round (csrc/lba_device.hip: reset_state).  State buffer 0 is restored from the upload;
of buffer 1 only the fixed keyframes' poses are read before a kernel has written them, and those are put there once per upload.  The
number of active windows, which the host once fetched from the device before queueing the first round, is counted on the host.
  * upload, optimize, optimize: the second call starts from the uploaded estimates again, whatever the first left in both buffers
  * a window gives the same bits after the context has solved a larger, different batch (its buffers then hold that batch's states)
  * a call in which no window is active (max_iterations == 0 everywhere; every stop flag set) returns its inputs and comes back."""
import numpy as np
import pytest

from orb_slam3_study_kr_amd import lba, synth

pytestmark = pytest.mark.gpu

FIELDS = ("chi2_trace", "lambda_trace", "trials_trace", "pose_qt", "points", "edge_chi2", "edge_depth_pos")


def _same(a, b):
    assert (a.iterations, a.trials) == (b.iterations, b.trials)
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


def _batch():
    # accepted and rejected trials (the second window: the rejection fixture of tests/test_gpu_lba.py), fixed keyframes in every
    # window, one window that is never active
    return [synth.make_window(9401, n_free=4, n_fixed=2, n_points=200, stereo=True, track_len=(2, 5)),
            synth.make_window(64, n_free=5, n_fixed=2, n_points=120, stereo=True, track_len=(2, 6), pose_noise=(0.08, 0.4), point_noise=1.5,
                              lambda_init=1e-4),
            synth.make_window(9402, n_free=3, n_fixed=3, n_points=90, stereo=False, track_len=(2, 4), max_iterations=0),
            synth.make_window(9403, n_free=9, n_fixed=1, n_points=300, stereo=True, track_len=(3, 9), max_iterations=4)]


def test_optimize_twice_gives_the_same_result(hip_lib):
    ws = _batch()
    with lba.LbaSolver(0) as s:
        s.upload(ws)
        s.optimize()
        first = s.download()
        s.optimize()
        second = s.download()
    assert any((r.trials_trace > 1).any() for r in first) and first[2].iterations == 0 and first[0].iterations > 1
    for a, b in zip(first, second):
        _same(a, b)


def test_a_window_after_a_larger_different_batch(hip_lib):
    ws = _batch()
    big = [synth.make_window(9410 + k, n_free=6 + k, n_fixed=2 + k % 3, n_points=500 + 60 * k, stereo=bool(k % 2), track_len=(2, 5 + k)) for k in range(6)]
    with lba.LbaSolver(0) as fresh:
        alone = [fresh.solve([w])[0] for w in ws[:2]]       # (each context's first and second solve)
    with lba.LbaSolver(0) as s:
        s.solve(big)
        after = [s.solve([ws[0]])[0]]
        s.solve(big[::-1])
        after.append(s.solve([ws[1]])[0])
        whole = s.solve(ws)
        s.solve(big)
        whole_again = s.solve(ws)
    for a, b in zip(alone, after):
        assert a.iterations > 1
        _same(a, b)
    for a, b in zip(whole, whole_again):
        _same(a, b)


def test_a_call_without_an_active_window_returns_its_inputs(hip_lib):
    ws = [synth.make_window(9420 + k, n_free=3 + k, n_fixed=2, n_points=60 + 30 * k, stereo=bool(k % 2), track_len=(2, 5), max_iterations=0) for k in range(5)]
    stopped = [synth.make_window(9430 + k, n_free=3, n_fixed=2, n_points=50, track_len=(2, 5)) for k in range(3)]
    for w in stopped:
        w.stop_flag = np.ones(1, dtype=np.uint8)
    with lba.LbaSolver(0) as s:
        s.solve([synth.make_window(9440, n_free=8, n_fixed=2, n_points=400, stereo=True, track_len=(2, 6))])   # leaves its states behind
        for batch in (ws, stopped, ws + stopped):
            for w, g in zip(batch, s.solve(batch)):
                assert g.iterations == 0 and g.trials == 0
                np.testing.assert_array_equal(g.points, w.points)
                np.testing.assert_array_equal(g.pose_qt[:, 4:], w.pose_qt[:w.n_free, 4:])
                # (the upload stores the rotation as g2o::SE3Quat does, normalised: the same rotation, not the same bits)
                q_in = w.pose_qt[:w.n_free, :4] / np.linalg.norm(w.pose_qt[:w.n_free, :4], axis=1, keepdims=True)
                np.testing.assert_allclose(np.abs(np.sum(g.pose_qt[:, :4] * q_in, axis=1)), 1.0, rtol=0, atol=1e-14)
                assert not g.edge_chi2.any()
