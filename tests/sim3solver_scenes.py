"""What the Sim3Solver class tests share (tests/test_sim3solver_class_cpu.py, tests/test_gpu_sim3solver_class.py): the scenes, the
Python restatement of the constructor, the minimal-set draw from a given RandomInt sequence, and the per-iteration results of the
host build that the Python replay steps over."""
import ctypes as C
import dataclasses

import numpy as np

import sim3_ransac_cases as sc
from orb_slam3_study_kr_amd import host, orb
from orb_slam3_study_kr_amd import synth_sim3_ransac as ss

LIBC = C.CDLL(None)
LIBC.rand.restype = C.c_int
RAND_MAX = 2147483647
F = np.float32


def problem(n=40, seed=3, fix_scale=True, cameras=(ss.PINHOLE, ss.PINHOLE), outliers=0.3):
    return ss.make_problem(seed=seed, n=n, iterations=0, camera_type1=cameras[0], camera_type2=cameras[1], fix_scale=fix_scale,
                           outlier_share=outliers)


def restate_constructor(scene):
    """src/Sim3Solver.cc:35-121 statement by statement on the arrays of a host.Sim3Scene (Pinhole cameras)."""
    passed_empty = scene.matched_kf is None
    bDifferentKFs = passed_empty                      # :40-45: set when the vector was passed EMPTY, and then filled with pKF2
    matched_kf = np.ones(scene.n1, np.int32) if passed_empty else scene.matched_kf
    pKFm = 1
    out = dict(x3dc1=[], x3dc2=[], max_error1=[], max_error2=[], indices1=[])
    for i1 in range(scene.n1):
        p2 = scene.matched12[i1]
        if p2 < 0:
            continue
        p1 = scene.kf1_mp[i1]
        if p1 < 0:
            continue
        if scene.bad[p1] or scene.bad[p2]:
            continue
        if bDifferentKFs:
            pKFm = int(matched_kf[i1])
        k1, k2 = scene.index_in_kf[p1, 0], scene.index_in_kf[p2, pKFm]
        if k1 < 0 or k2 < 0:
            continue
        out["max_error1"].append(ss.truncated_threshold(scene.level_sigma2[scene.octave[0][k1]]))
        out["max_error2"].append(ss.truncated_threshold(scene.level_sigma2[scene.octave[pKFm][k2]]))
        out["indices1"].append(i1)
        out["x3dc1"].append(ss.to_camera(scene.Rcw[0], scene.tcw[0], scene.world[p1][None])[0])
        out["x3dc2"].append(ss.to_camera(scene.Rcw[1], scene.tcw[1], scene.world[p2][None])[0])   # pKF2's pose, whatever pKFm is
    out = {k: np.asarray(v, np.int32 if k == "indices1" else F).reshape((-1, 3) if k.startswith("x3dc") else (-1,)) for k, v in out.items()}
    for cam, x, name in ((scene.camera[0], out["x3dc1"], "p1im1"), (scene.camera[1], out["x3dc2"], "p2im2")):
        out[name] = np.stack([cam[0] * x[:, 0] / x[:, 2] + cam[2], cam[1] * x[:, 1] / x[:, 2] + cam[3]], 1).astype(F)
    return out


def draw_sets(n, iterations, randi):
    """:172-186 with the RandomInt values handed in: a fresh copy of mvAllIndices per iteration, swap-with-back removal."""
    randi = iter(randi)
    sets = []
    for _ in range(iterations):
        avail = list(range(n))
        row = []
        for _ in range(3):
            r = next(randi)
            row.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        sets.append(row)
    return sets


def random_ints(n, iterations):
    """The values DUtils::Random::RandomInt(0, size - 1) returns for the draws of `iterations` sets, from the process's rand()."""
    return [int((LIBC.rand() / (RAND_MAX + 1.0)) * (n - j)) for _ in range(iterations) for j in range(3)]


def packed_problem(solver, sets):
    """The osh_sim3r_problem the solver's device call receives, as a synth Problem."""
    p, st = solver.pack(), solver.state()
    pb = solver.scene.pb
    return dataclasses.replace(pb, x3dc1=p["x3dc1"], x3dc2=p["x3dc2"], p1im1=p["p1im1"], p2im2=p["p2im2"], max_error1=p["max_error1"],
                               max_error2=p["max_error2"], sets=np.asarray(sets, np.int32).reshape(-1, 3), min_inliers=st["min_inliers"],
                               best_inliers_in=0)


def per_iteration(pb):
    """counts, transforms and flags of every iteration from the host build."""
    o = orb.sim3_ransac_cpu([pb], debug=True)[0][0]
    rec = {int(k): q for q, k in enumerate(o["record"][:int(o["n_records"][0])])}
    flags_of_records = sc.mask_bits(o["record_mask"], pb.n)[0]
    flags = np.zeros((len(pb.sets), pb.n), bool)
    for k, q in rec.items():
        flags[k] = flags_of_records[q]
    return o["debug_count"], o["debug_T"], flags


def assert_same_step(got, want, what):
    assert (got["no_more"], got["converged"], got["n_inliers"]) == (want["no_more"], want["converged"], want["n_inliers"]), what
    assert np.array_equal(got["inliers"], want["inliers"]), what
    assert np.array_equal(got["T12"].view(np.uint32), want["T12"].view(np.uint32)), what


def twin_sets(scene, ransac, seed):
    """The sets a solver of this scene draws after srand(seed): drawn on a twin, so that the solver under test draws them itself."""
    with host.Sim3Solver(scene, ransac=ransac) as twin:
        LIBC.srand(seed)
        return twin.prepare()
