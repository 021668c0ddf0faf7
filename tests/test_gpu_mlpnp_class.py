"""The drop-in MLPnPsolver class on the device: iterate end to end against the generator's truth, a second iterate after a returned
pose, a round beyond the entry's limits answered by the host build with the same decision, and MLPnPsolver::IterateBatch of five
solvers against five single calls."""
import ctypes as C

import numpy as np
import pytest

import mlpnp_cases as mc
import mlpnp_numpy as mn
from orb_slam3_study_kr_amd import host
from orb_slam3_study_kr_amd import synth_mlpnp as sm

pytestmark = pytest.mark.gpu

LIBC = C.CDLL(None)
F32 = float(np.finfo(np.float32).eps)


def pose_of(T):
    return np.concatenate([T[:3, :3].astype(np.float64).reshape(9), T[:3, 3].astype(np.float64)])


@pytest.mark.parametrize("camera", (sm.PINHOLE, sm.KB8))
def test_iterate_end_to_end_and_again(hip_lib, camera):
    """300 points, 50 % outliers: iterate returns true with the refined pose, every true inlier flagged and no outlier; a second
    iterate continues from the stored state (the queue of unused sets, mnIterations, the best and its cached Refine)."""
    pb = mc.end_to_end(camera, 0.5)
    LIBC.srand(0)
    with host.MlpnpSolver(pb, extra=3, bad=2) as s:
        r = s.iterate(5)
        st = s.state()
        assert r["found"] and not r["no_more"] and st["on_device"] == 1
        assert r["inliers"].shape == (305,) and np.array_equal(r["inliers"][3:303], pb.inlier) and not r["inliers"][:3].any() and not r["inliers"][303:].any()
        assert r["n_inliers"] == pb.inlier.sum()
        rot, trans = mn.pose_difference(pose_of(r["Tout"]), pb.pose)
        # twice the numpy restatement's own error against truth, and the float32 conversion of Tout (entries up to 6 in size)
        assert rot <= 2 * mc.NUMPY_VS_TRUTH[camera][0] + 8 * F32 and trans <= 2 * mc.NUMPY_VS_TRUTH[camera][1] + 8 * 6 * F32
        assert np.array_equal(r["Tout"][3], [0, 0, 0, 1])
        assert 0 < st["iterations"] <= 70 and st["iterations"] + st["queued_sets"] == 70 and st["best_inliers"] >= st["min_inliers"] == 120
        r2 = s.iterate(5)
        st2 = s.state()
        assert r2["found"] and st2["on_device"] == 1 and st2["iterations"] > st["iterations"] and st2["best_inliers"] >= st["best_inliers"]
        assert st2["iterations"] + st2["queued_sets"] == 70   # the second call ran on the queued sets and drew none
        assert np.array_equal(r2["inliers"], r["inliers"])
        if r2["no_more"]:   # no further set reached min_inliers: the best (a hypothesis, not its refinement) is returned at exhaustion
            assert st2["iterations"] == 70 and r2["n_inliers"] == st2["best_inliers"]


def test_second_iterate_answers_from_the_stored_state(hip_lib):
    """20 % outliers, so that many sets reach min_inliers: after a returned pose the next iterate returns at its first such set with
    the cached Refine of the unchanged best, or with the Refine of a new record."""
    pb = sm.make_problem(seed=6, n=300, iterations=0, outlier_share=0.2)
    LIBC.srand(0)
    with host.MlpnpSolver(pb) as s:
        r = s.iterate(5)
        st = s.state()
        r2 = s.iterate(5)
        st2 = s.state()
        assert r["found"] and r2["found"] and not r["no_more"] and not r2["no_more"] and st["on_device"] == st2["on_device"] == 1
        assert st["iterations"] < st2["iterations"] < 70 and st2["iterations"] + st2["queued_sets"] == 70
        assert np.array_equal(r["inliers"], pb.inlier) and np.array_equal(r2["inliers"], pb.inlier)
        if st2["best_inliers"] == st["best_inliers"]:   # the best was not beaten: its cached Refine answered
            assert np.array_equal(r2["Tout"], r["Tout"]) and r2["n_inliers"] == r["n_inliers"]
        assert mn.pose_difference(pose_of(r2["Tout"]), pb.pose)[1] <= 1e-2


def test_a_round_beyond_the_limits_is_answered_by_the_host_build_with_the_same_decision(hip_lib):
    pb = mc.end_to_end(sm.PINHOLE, 0.5)
    LIBC.srand(0)
    with host.MlpnpSolver(pb) as s:
        dev = s.iterate(5)
        st_dev = s.state()
    LIBC.srand(0)
    with host.MlpnpSolver(pb) as s:
        cpu = s.iterate(1025)   # 1025 iterations in one round: more than OSH_MLPNP_MAX_ITERATIONS
        st_cpu = s.state()
    assert st_dev["on_device"] == 1 and st_cpu["on_device"] == 0
    assert dev["found"] and cpu["found"] and st_cpu["iterations"] == st_dev["iterations"] and st_cpu["best_inliers"] == st_dev["best_inliers"]
    assert st_cpu["queued_sets"] == 1025 - st_cpu["iterations"]
    assert np.array_equal(dev["inliers"], cpu["inliers"]) and dev["n_inliers"] == cpu["n_inliers"]
    assert np.abs(dev["Tout"] - cpu["Tout"]).max() <= 4 * 6 * F32
    big = sm.make_problem(seed=9, n=2049, iterations=0, outlier_share=0.2)   # more than OSH_MLPNP_MAX_POINTS correspondences
    LIBC.srand(0)
    with host.MlpnpSolver(big) as s:
        r = s.iterate(5)
        assert s.state()["on_device"] == 0 and r["found"] and np.array_equal(r["inliers"], big.inlier)


def test_iterate_batch_equals_single_calls(hip_lib):
    pbs = [mc.end_to_end(sm.PINHOLE, 0.5), sm.make_problem(seed=31, n=65, camera_type=sm.KB8, outlier_share=0.3, iterations=0),
           sm.make_problem(seed=32, n=7, iterations=0), sm.make_problem(seed=33, n=130, outlier_share=0.6, iterations=0), mc.end_to_end(sm.KB8, 0.5)]

    def run(batch):
        LIBC.srand(0)
        solvers = [host.MlpnpSolver(pb, extra=k) for k, pb in enumerate(pbs)]
        try:
            first = host.mlpnp_iterate(solvers, 5, batch=batch)
            second = host.mlpnp_iterate(solvers, 5, batch=batch)
            return first, second, [s.state() for s in solvers]
        finally:
            for s in solvers:
                s.close()

    a, b = run(True), run(False)
    assert a[2] == b[2]
    for ra, rb in zip(a[0] + a[1], b[0] + b[1]):
        assert ra.keys() == rb.keys()
        for k in ra:
            assert np.array_equal(np.atleast_1d(np.asarray(ra[k])).view(np.uint8), np.atleast_1d(np.asarray(rb[k])).view(np.uint8)), k
    assert a[0][0]["found"] and a[0][4]["found"]
    assert a[0][2]["no_more"] and not a[0][2]["found"]   # 7 correspondences, 8 inliers asked for
    assert all(st["on_device"] == 1 for k, st in enumerate(a[2]) if k != 2)
