"""The drop-in MLPnPsolver class (include/MLPnPsolver.h, csrc/host/MLPnPsolver.cc) without a device: the constructor's selection of
correspondences, SetRansacParameters as Tracking::Relocalization calls it, the minimal-set draw, and the replay of a device answer
(Prepare / Replay around the one device call) from synthetic answers: the early return at the first hit, the cached Refine of an
earlier best across two iterate calls, exhaustion with and without a best, the OR of the reference's loop bound and the queue of
unused sets."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_study_kr_amd import host
from orb_slam3_study_kr_amd import synth_mlpnp as sm

LIBC = C.CDLL(None)
LIBC.rand.restype = C.c_int
RAND_MAX = 2147483647


def scene(n, seed=3, camera=sm.PINHOLE):
    return sm.make_problem(seed=seed, n=n, iterations=0, camera_type=camera, outlier_share=0.3)


@pytest.mark.parametrize("n,min_inliers,max_iterations", [(9, 10, 1), (10, 10, 1), (11, 10, 4), (20, 10, 35), (300, 150, 35)])
def test_relocalisation_parameters(n, min_inliers, max_iterations):
    with host.MlpnpSolver(scene(n), relocalisation=True) as s:
        st = s.state()
        assert (st["N"], st["min_inliers"], st["max_iterations"]) == (n, min_inliers, max_iterations)
        if n == 9:   # fewer correspondences than inliers asked for: iterate gives up at once, whatever the device
            r = s.iterate(5)
            assert not r["found"] and r["no_more"] and r["n_inliers"] == 0 and not r["has_inliers"]
            assert np.array_equal(r["Tout"], np.eye(4, dtype=np.float32)) and s.state()["iterations"] == 0


def test_constructor_defaults_and_the_correspondences_it_keeps():
    pb = scene(40)
    with host.MlpnpSolver(pb, extra=7, bad=5) as s:
        st = s.state()
        assert (st["N"], st["min_inliers"], st["max_iterations"]) == (40, 16, 70)   # 40 * 0.4; ceil(log(0.01) / log(1 - 0.064)) = 70
        assert s.n_matches == 52
        sets, count = s.prepare(3)
        assert count == 70 and sets.min() >= 0 and sets.max() < 40
        assert all(len(set(row)) == 6 for row in sets.tolist())
        flags = np.zeros(40, bool); flags[[0, 5, 39]] = True
        r = s.replay(first_hit=0, hit_record=0, hit_count=17, best_iteration=0, best_count=17, best_refine_ok=1, hit_pose=pb.pose, hit_flags=flags,
                     best_pose=pb.pose, best_flags=flags)
        # vbInliers has one entry per vpMapPointMatches entry and is set through mvKeyPointIndices: the 7 leading entries are skipped
        assert r["found"] and r["inliers"].shape == (52,) and list(np.flatnonzero(r["inliers"])) == [7, 12, 46]
        want = np.eye(4, dtype=np.float32)
        want[:3, :3], want[:3, 3] = pb.pose[:9].reshape(3, 3).astype(np.float32), pb.pose[9:].astype(np.float32)
        assert np.array_equal(r["Tout"], want)


def test_sets_are_drawn_as_the_reference_draws_them():
    """RandomInt of DUtils and the swap-with-back removal over mvAllIndices, from the process's rand() stream."""
    with host.MlpnpSolver(scene(20), relocalisation=True) as s:
        LIBC.srand(0)
        sets, count = s.prepare(2)
        LIBC.srand(0)
        want = []
        for _ in range(count):
            avail = list(range(20))
            row = []
            for _ in range(6):
                d = len(avail)
                randi = int((LIBC.rand() / (RAND_MAX + 1.0)) * d)
                row.append(avail[randi])
                avail[randi] = avail[-1]
                avail.pop()
            want.append(row)
        assert count == 35 and sets.tolist() == want


def test_replay_across_calls():
    pb = scene(20)
    flags_best = np.zeros(20, bool); flags_best[:12] = True
    flags_ref = np.zeros(20, bool); flags_ref[:15] = True
    other = pb.pose.copy(); other[9:] += 0.25
    with host.MlpnpSolver(pb, extra=2, relocalisation=True) as s:
        # the OR of the loop condition: max(mRansacMaxIts - mnIterations, nIterations) iterations in one call
        sets1, count = s.prepare(5)
        assert count == 35
        # an early return at the first hit, iteration 2: three iterations consumed, 32 sets left over
        r = s.replay(first_hit=2, hit_record=0, hit_count=15, best_iteration=2, best_count=12, best_refine_ok=1, hit_pose=pb.pose,
                     hit_flags=flags_ref, best_pose=other, best_flags=flags_best)
        assert r["found"] and not r["no_more"] and r["n_inliers"] == 15 and list(np.flatnonzero(r["inliers"])) == list(range(2, 17))
        first_T = r["Tout"]
        st = s.state()
        assert (st["iterations"], st["best_inliers"], st["queued_sets"]) == (3, 12, 32)
        # the next call uses the queued sets first, in order
        sets2, count = s.prepare(5)
        assert count == 32 and np.array_equal(sets2, sets1[3:]) and s.state()["queued_sets"] == 0
        # iteration 1 has enough inliers and is no record: the Refine of the unchanged best answers again, from the solver's cache
        r = s.replay(first_hit=1, hit_record=-1, best_iteration=-1, best_count=12, best_refine_ok=1)
        assert r["found"] and r["n_inliers"] == 15 and np.array_equal(r["Tout"], first_T) and list(np.flatnonzero(r["inliers"])) == list(range(2, 17))
        st = s.state()
        assert (st["iterations"], st["best_inliers"], st["queued_sets"]) == (5, 12, 30)
        # exhaustion with a best: no hit in the remaining 30 iterations, mnIterations reaches mRansacMaxIts, the best is returned
        sets3, count = s.prepare(5)
        assert count == 30 and np.array_equal(sets3, sets1[5:])
        r = s.replay(best_iteration=-1, best_count=12, best_refine_ok=1)
        assert r["found"] and r["no_more"] and r["n_inliers"] == 12 and list(np.flatnonzero(r["inliers"])) == list(range(2, 14))
        assert np.allclose(r["Tout"][:3, 3], other[9:].astype(np.float32), rtol=0, atol=0)
        assert s.state()["iterations"] == 35
        # past mRansacMaxIts the caller's nIterations is what one call runs
        sets4, count = s.prepare(5)
        assert count == 5 and s.state()["queued_sets"] == 0
        r = s.replay(best_iteration=-1, best_count=12, best_refine_ok=1)
        assert r["found"] and r["no_more"] and s.state()["iterations"] == 40


def test_exhaustion_without_a_best_and_a_failed_refine():
    with host.MlpnpSolver(scene(20), relocalisation=True) as s:
        sets, count = s.prepare(5)
        r = s.replay()
        assert not r["found"] and r["no_more"] and r["n_inliers"] == 0 and not r["has_inliers"] and s.state()["iterations"] == 35
    flags = np.zeros(20, bool); flags[:11] = True
    with host.MlpnpSolver(scene(20), relocalisation=True) as s:
        s.set_ransac(0.99, 10, 300, 6, 0.5, 5.991)
        s.prepare(5)
        # a record whose Refine fails: the best is stored, nothing is returned before exhaustion, then the best is
        r = s.replay(best_iteration=4, best_count=11, best_refine_ok=0, best_pose=scene(20).pose, best_flags=flags)
        assert r["found"] and r["no_more"] and r["n_inliers"] == 11 and s.state()["best_inliers"] == 11
