"""The drop-in Sim3Solver class on the device: the caller's loop on the scenes of tests/test_sim3solver_class_cpu.py gives what the
Python replay gives over the host build's per-iteration results (which is what the class gives on its host path, as the CPU file
shows), mbLastOnDevice is set, Sim3Solver::IterateBatch of five solvers equals five iterate calls, and a problem beyond
OSH_SIM3R_MAX_POINTS is answered by the host build after a message."""
import numpy as np
import pytest

import sim3_ransac_cases as sc
import sim3_ransac_numpy as s3n
from orb_slam3_study_kr_amd import capi, host
from orb_slam3_study_kr_amd import synth_sim3_ransac as ss
from sim3solver_scenes import LIBC, assert_same_step, packed_problem, per_iteration, problem, twin_sets

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fix_scale,cameras,min_inliers,seed", [(True, (ss.PINHOLE, ss.PINHOLE), 20, 5), (False, (ss.PINHOLE, ss.PINHOLE), 20, 6),
                                                                (False, (ss.KB8, ss.PINHOLE), 25, 7), (True, (ss.PINHOLE, ss.PINHOLE), 20, 8)])
def test_the_callers_loop_on_the_device_equals_the_host_path(hip_lib, fix_scale, cameras, min_inliers, seed):
    pb = problem(40, seed=seed, fix_scale=fix_scale, cameras=cameras, outliers=0.7 if seed == 8 else 0.3)
    scene = host.Sim3Scene(pb, extra=4, seed=seed, null_match=(1,), bad2=(2,))
    ransac = (0.99, min_inliers, 300)
    sets = twin_sets(scene, ransac, seed)
    with host.Sim3Solver(scene, ransac=ransac) as s:
        st = s.state()
        count, T, flags = per_iteration(packed_problem(s, sets))
        ref = s3n.Replay(st["N"], st["n1"], s.pack()["indices1"], st["min_inliers"], st["max_iterations"])
        LIBC.srand(seed)
        calls = 0
        while True:
            got, want = s.iterate(20), ref.iterate(20, count, T, flags)
            calls += 1
            assert_same_step(got, want, f"call {calls}")
            st = s.state()
            assert (st["iterations"], st["best_inliers"], st["on_device"], st["has_answer"]) == (ref.iterations, ref.best_inliers, 1, 1)
            if got["converged"] or got["no_more"]:
                break
        assert got["no_more"] if seed == 8 else got["converged"]
        if ref.best_T is not None:
            b = s.best()
            assert np.array_equal(b["flags"], ref.best_flags) and np.array_equal(np.concatenate([b["R"].reshape(9), b["t"], b["s"]]), ref.best_T)


def test_end_to_end_against_the_truth(hip_lib):
    pb = sc.end_to_end(2, False)
    LIBC.srand(0)
    with host.Sim3Solver(host.Sim3Scene(pb, extra=3), ransac=(0.99, 15, 300)) as s:
        r = s.iterate(300)
        assert r["converged"] and r["n_inliers"] > 15 and s.state()["on_device"] == 1
        b = s.best()
        d = sc.truth_difference(pb, np.concatenate([b["R"].reshape(9), b["t"], b["s"]]))
        assert all(x <= y for x, y in zip(d, sc.TRUTH_BOUND)), d
        idx = s.pack()["indices1"]
        assert not (r["inliers"][idx] & ~pb.inlier).any() and r["inliers"].sum() == r["n_inliers"]


def test_iterate_batch_of_five_equals_five_iterate_calls(hip_lib):
    scenes = [host.Sim3Scene(problem(n, seed=30 + k, fix_scale=k % 2 == 0, cameras=cams), extra=k, seed=k)
              for k, (n, cams) in enumerate([(40, (ss.PINHOLE, ss.PINHOLE)), (65, (ss.KB8, ss.KB8)), (5, (ss.PINHOLE, ss.PINHOLE)),
                                             (100, (ss.PINHOLE, ss.KB8)), (64, (ss.PINHOLE, ss.PINHOLE))])]
    ransacs = [(0.99, 20, 300), (0.99, 30, 300), (0.99, 6, 300), (0.99, 40, 50), (0.99, 20, 300)]   # the third has N < minInliers
    single, batch = [], []
    solvers = [host.Sim3Solver(sc_, ransac=r) for sc_, r in zip(scenes, ransacs)]
    try:
        LIBC.srand(3)
        for _ in range(3):
            single.append([s.iterate(20) for s in solvers])
        states = [s.state() for s in solvers]
    finally:
        for s in solvers:
            s.close()
    solvers = [host.Sim3Solver(sc_, ransac=r) for sc_, r in zip(scenes, ransacs)]
    try:
        # one by one the solvers draw in turn on their first call; the batch draws in the same order before its one device call
        LIBC.srand(3)
        for _ in range(3):
            batch.append(host.sim3_iterate(solvers, 20, mode=2))
        for k, s in enumerate(solvers):
            assert s.state() == states[k], f"solver {k}"
            assert s.state()["on_device"] == (0 if k == 2 else 1)
    finally:
        for s in solvers:
            s.close()
    for call, (a, b) in enumerate(zip(single, batch)):
        for k, (x, y) in enumerate(zip(a, b)):
            assert_same_step(y, x, f"call {call}, solver {k}")
    assert single[0][2]["no_more"] and any(r["converged"] for r in single[0])


def test_beyond_the_point_limit_the_host_answers(hip_lib, capfd):
    pb = ss.make_problem(seed=4, n=capi.OSH_SIM3R_MAX_POINTS + 4, iterations=0, outlier_share=0.3)
    scene = host.Sim3Scene(pb, extra=0)
    ransac = (0.99, 2000, 8)
    sets = twin_sets(scene, ransac, 1)
    with host.Sim3Solver(scene, ransac=ransac) as s:
        st = s.state()
        assert st["N"] == capi.OSH_SIM3R_MAX_POINTS + 4 and st["max_iterations"] == 8
        count, T, flags = per_iteration(packed_problem(s, sets))
        ref = s3n.Replay(st["N"], st["n1"], s.pack()["indices1"], st["min_inliers"], st["max_iterations"])
        LIBC.srand(1)
        capfd.readouterr()
        got = s.iterate(8)
        assert "beyond the device limits; running on the host" in capfd.readouterr().err
        assert_same_step(got, ref.iterate(8, count, T, flags), "host answer")
        assert s.state()["on_device"] == 0 and s.state()["has_answer"] == 1
