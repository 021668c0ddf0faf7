"""The host build of csrc/sim3_ransac.h (the statements osh_orb_sim3_ransac runs on the device) against the numpy restatement of
Sim3Solver (tests/sim3_ransac_numpy.py): the whole pipeline away from the thresholds, CheckInliers for Pinhole pairs bit for bit, the
hypotheses of well-conditioned minimal sets within the measured bound, degenerate sets, the size_t truncation of the thresholds, both
scale modes, the end-to-end scenes against the generator's truth, and the refusals of the entry (which need no device)."""
import dataclasses

import numpy as np
import pytest

import sim3_ransac_cases as sc
import sim3_ransac_numpy as s3n
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_sim3_ransac as ss


# ------------------------------------------------------------------------------------------------------------ scoring
@pytest.mark.parametrize("fix_scale", (True, False))
@pytest.mark.parametrize("n", sc.SIZES)
def test_scoring_pinhole_equals_numpy_bit_for_bit(n, fix_scale):
    pb = sc.grid_problem(n, 1, "pinhole-pinhole", fix_scale)
    Ts = sc.transforms(pb, n)
    count, mask = orb.sim3_ransac_check_inliers_cpu(pb, Ts)
    flags, clean = sc.mask_bits(mask, n)
    assert clean
    for k, T in enumerate(Ts):
        want, c = s3n.check_inliers(pb, T)
        assert np.array_equal(flags[k], want), f"transform {k}"
        assert count[k] == c
    assert count[0] == pb.inlier.sum() and count[-1] < max(count[0], 1)   # from all found to almost none
    if n >= 63:
        assert 0 < count[2] and len(set(count.tolist())) >= 3, count


@pytest.mark.parametrize("cameras", ("kb8-kb8", "pinhole-kb8"))
def test_scoring_kb8_equals_numpy_away_from_the_threshold(cameras):
    pb = sc.grid_problem(300, 1, cameras, False)
    Ts = sc.transforms(pb, 5)[:3]
    want = []
    for T in Ts:
        assert s3n.threshold_margin(pb, T) > sc.THRESHOLD_MARGIN, "a point lies near its threshold"
        want.append(s3n.check_inliers(pb, T)[0])
    count, mask = orb.sim3_ransac_check_inliers_cpu(pb, Ts)
    assert np.array_equal(sc.mask_bits(mask, pb.n)[0], np.stack(want)) and np.array_equal(count, np.stack(want).sum(1))
    assert np.array_equal(want[0], pb.inlier)


# ------------------------------------------------------------------------------------------------------------ hypotheses
def test_hypotheses_against_numpy():
    worst = 0.0
    for pb, ref in sc.hypothesis_cases():
        for s in pb.sets:
            assert min(ss.triangle_quality(pb.x3dc1[s]), ss.triangle_quality(pb.x3dc2[s])) >= sc.MIN_QUALITY
        out = orb.sim3_ransac_cpu([pb], debug=True)[0][0]
        worst = max(worst, sc.hypothesis_difference(out["debug_T"], ref))
        # the stage wrapper runs the same statement
        T0 = orb.sim3_ransac_stage("compute_sim3", pb.x3dc1[pb.sets[0]], pb.x3dc2[pb.sets[0]], pb.fix_scale)
        assert np.array_equal(T0.view(np.uint32), out["debug_T"][0].view(np.uint32))
        if pb.fix_scale:
            assert (out["debug_T"][:, 12] == 1.0).all()
        else:
            assert (out["debug_T"][:, 12] != 1.0).any()
    print(f"host build against numpy over the hypothesis cases: {worst:.3g}")
    assert worst <= sc.HYPOTHESIS_BOUND


def test_rotation_is_a_rotation_and_the_identity_gives_no_nan():
    pb = sc.hypothesis_cases()[1][0]
    T = orb.sim3_ransac_cpu([pb], debug=True)[0][0]["debug_T"].astype(np.float64)
    for Tk in T:
        R = Tk[:9].reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() < 4e-7 and abs(np.linalg.det(R) - 1) < 4e-7   # float32 entries of an FP64 rotation
    # both sets equal: the quaternion is (1, 0, 0, 0), where the reference divides by vec.norm() = 0
    P = pb.x3dc1[pb.sets[0]]
    Tid = orb.sim3_ransac_stage("compute_sim3", P, P, False)
    assert np.array_equal(Tid[:9].reshape(3, 3), np.eye(3, dtype=np.float32)) and np.isfinite(Tid).all()
    assert abs(Tid[12] - 1) < 1e-6 and np.abs(Tid[9:12]).max() < 1e-5


@pytest.mark.parametrize("kind", ("collinear", "coincident", "zero_den"))
def test_degenerate_sets(kind):
    pb = ss.with_degenerate_set(sc.grid_problem(65, 3, "pinhole-pinhole", False), kind)
    out = orb.sim3_ransac_cpu([pb], debug=True)[0][0]
    assert np.isfinite(out["debug_T"][0, :9]).all()
    sc.assert_self_consistent(pb, out)
    if kind == "zero_den":
        assert not np.isfinite(out["debug_T"][0, 12]) and out["debug_count"][0] == 0
        # the iterations behind it are those of the problem without the degenerate set
        ref = orb.sim3_ransac_cpu([dataclasses.replace(pb, sets=pb.sets[1:])], debug=True)[0][0]
        assert np.array_equal(out["debug_count"][1:], ref["debug_count"])
    # with a fixed scale the zero denominator is never formed
    fixed = orb.sim3_ransac_cpu([dataclasses.replace(pb, fix_scale=1)], debug=True)[0][0]
    assert np.isfinite(fixed["debug_T"][0]).all() and fixed["debug_T"][0, 12] == 1.0


def test_nan_coordinate_ends_in_zero_inliers():
    pb = sc.grid_problem(65, 3, "pinhole-pinhole", True)
    x = pb.x3dc2.copy(); x[pb.sets[1, 0], 1] = np.nan
    out = orb.sim3_ransac_cpu([dataclasses.replace(pb, x3dc2=x)], debug=True)[0][0]
    assert out["debug_count"][1] == 0
    sc.assert_self_consistent(pb, out)


def test_thresholds_are_truncated_as_size_t():
    assert float(ss.truncated_threshold(np.float32(1.44))) == 13.0          # 9.210 * 1.44 = 13.26
    pb = sc.grid_problem(64, 1, "pinhole-pinhole", True)
    truth = np.concatenate([pb.R12.reshape(9), pb.t12, [pb.s12]]).astype(np.float32)
    # an error between the truncated and the untruncated threshold is an outlier under the first and an inlier under the second
    i = int(np.flatnonzero(pb.inlier)[0])
    for thr, want in ((np.float32(13.0), False), (np.float32(13.26), True)):
        m1 = pb.max_error1.copy(); m1[i] = thr
        x = dataclasses.replace(pb, max_error1=m1, p1im1=pb.p1im1.copy())
        x.p1im1[i, 0] += np.float32(np.sqrt(13.1))                          # err1 = 13.1 up to the point's own residual
        err = s3n.errors(x, truth)[0][i]
        assert 13.0 < err < 13.26
        count, mask = orb.sim3_ransac_check_inliers_cpu(x, truth)
        assert bool(sc.mask_bits(mask, pb.n)[0][0, i]) is want


# ------------------------------------------------------------------------------------------------------------ the whole pipeline
@pytest.mark.parametrize("cameras,fix_scale,seed", [("pinhole-pinhole", True, 7), ("pinhole-pinhole", False, 7), ("kb8-kb8", False, 8), ("pinhole-kb8", True, 7)])
def test_pipeline_equals_numpy_away_from_the_threshold(cameras, fix_scale, seed):
    pb = dataclasses.replace(sc.grid_problem(65, 300, cameras, fix_scale, seed), min_inliers=30)
    pb = dataclasses.replace(pb, sets=pb.sets[:40])
    ref = s3n.solve(pb)
    assert min(s3n.threshold_margin(pb, T) for T in ref["T"]) > sc.THRESHOLD_MARGIN, "a correspondence lies near its threshold"
    out = orb.sim3_ransac_cpu([pb], debug=True)[0][0]
    sc.assert_self_consistent(pb, out)
    assert np.array_equal(out["debug_count"], ref["count"])
    n_rec = int(out["n_records"][0])
    assert list(out["record"][:n_rec]) == ref["record"] and int(out["first_hit"][0]) == ref["first_hit"]
    assert int(out["best_iteration"][0]) == ref["best_iteration"] and int(out["best_count"][0]) == ref["best_count"]
    assert np.array_equal(sc.mask_bits(out["record_mask"], pb.n)[0][:n_rec], ref["flags"][ref["record"]])
    assert sc.hypothesis_difference(out["debug_T"], ref["T"]) <= 1e-5   # sets of any shape: not the bound of the well-conditioned list


def test_records_from_synthetic_counts():
    count = [3, 3, 2, 7, 7, 9, 1, 9, 12, 12, 4]
    for min_inliers, best_in in ((6, 0), (8, 0), (20, 0), (6, 7), (6, 9), (6, 13), (11, 3)):
        record, res = orb.sim3_ransac_stage("scan", count, min_inliers, best_in)
        want = s3n.scan(count, min_inliers, best_in)
        assert list(record) == want["record"]
        assert list(res) == [want["first_hit"], len(want["record"]), want["best_iteration"], want["best_count"]]
    # ties go to the later iteration, and the running best goes on across a hit
    record, res = orb.sim3_ransac_stage("scan", count, 6, 0)
    assert list(record) == [0, 1, 3, 4, 5, 7, 8, 9] and list(res) == [3, 8, 9, 12]


@pytest.mark.parametrize("fix_scale", (True, False))
@pytest.mark.parametrize("seed", sc.END_TO_END_SEEDS)
def test_end_to_end_numpy_reaches_a_hit(seed, fix_scale):
    pb, ref = sc.end_to_end(seed, fix_scale), sc.end_to_end_numpy(seed, fix_scale)
    assert ref["first_hit"] >= 0
    d = sc.truth_difference(pb, ref["T"][ref["first_hit"]])
    print(f"seed {seed}, fix_scale {fix_scale}: numpy against the truth {d}")
    assert all(a <= b for a, b in zip(d, sc.NUMPY_VS_TRUTH))


@pytest.mark.parametrize("fix_scale", (True, False))
@pytest.mark.parametrize("seed", sc.END_TO_END_SEEDS)
def test_end_to_end_against_the_truth(seed, fix_scale):
    pb = sc.end_to_end(seed, fix_scale)
    out = orb.sim3_ransac_cpu([pb], debug=True)[0][0]
    hit = int(out["first_hit"][0])
    assert hit >= 0 and out["debug_count"][hit] > pb.min_inliers
    q = list(out["record"]).index(hit)
    d = sc.truth_difference(pb, out["record_T"][q])
    assert all(a <= b for a, b in zip(d, sc.TRUTH_BOUND)), d
    flags = sc.mask_bits(out["record_mask"], pb.n)[0][q]
    assert not (flags & ~pb.inlier).any()          # no outlier is taken for an inlier
    sc.assert_self_consistent(pb, out)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_need_no_device():
    lib = capi.load_library()
    pb = sc.grid_problem(65, 3, "pinhole-pinhole", True)
    repeats = pb.sets.copy(); repeats[1, 2] = repeats[1, 0]
    outside = pb.sets.copy(); outside[2, 0] = pb.n
    negative = pb.sets.copy(); negative[0, 1] = -1
    small = sc.grid_problem(3, 1, "pinhole-pinhole", True)
    two = dataclasses.replace(small, x3dc1=small.x3dc1[:2], x3dc2=small.x3dc2[:2], p1im1=small.p1im1[:2], p2im2=small.p2im2[:2],
                              max_error1=small.max_error1[:2], max_error2=small.max_error2[:2])
    big = ss.make_problem(seed=2, n=capi.OSH_SIM3R_MAX_POINTS + 1, iterations=1)
    bad = [(dataclasses.replace(pb, sets=repeats), "set 1 repeats index", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, sets=outside), "set 2: index 65 outside", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, sets=negative), "index -1 outside", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, camera_type1=2), "camera type 2", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, camera_type2=-1), "camera type -1", capi.OSH_ERR_INVALID),
           (two, "2 correspondences cannot fill a minimal set of 3", capi.OSH_ERR_INVALID),
           (big, "more than 4096 correspondences", capi.OSH_ERR_UNSUPPORTED),
           (dataclasses.replace(pb, sets=np.tile(pb.sets, (342, 1))), "more than 1024 iterations", capi.OSH_ERR_UNSUPPORTED)]
    for problem, message, code in bad:
        cp, cr, _keep, _outs = orb.sim3_ransac_args([pb, problem])
        assert lib.osh_orb_sim3_ransac(None, 2, cp, cr) == code
        assert message in capi.last_error(lib) and "problem 1" in capi.last_error(lib)
    cp, cr, _keep, _outs = orb.sim3_ransac_args([pb])
    cp[0].n = -1
    assert lib.osh_orb_sim3_ransac(None, 1, cp, cr) == capi.OSH_ERR_INVALID and "negative count" in capi.last_error(lib)
    cp, cr, _keep, _outs = orb.sim3_ransac_args([pb])
    cp[0].n_iterations = -2
    assert lib.osh_orb_sim3_ransac(None, 1, cp, cr) == capi.OSH_ERR_INVALID and "negative count" in capi.last_error(lib)
    cp, cr, _keep, _outs = orb.sim3_ransac_args([pb])
    cp[0].p2im2 = None
    assert lib.osh_orb_sim3_ransac(None, 1, cp, cr) == capi.OSH_ERR_INVALID and "NULL array with n = 65" in capi.last_error(lib)
    cp, cr, _keep, _outs = orb.sim3_ransac_args([pb])
    cp[0].sets = None
    assert lib.osh_orb_sim3_ransac(None, 1, cp, cr) == capi.OSH_ERR_INVALID and "NULL sets" in capi.last_error(lib)
    assert lib.osh_orb_sim3_ransac(None, -1, cp, cr) == capi.OSH_ERR_INVALID
    cp, cr, _keep, _outs = orb.sim3_ransac_args([pb] * (capi.OSH_SIM3R_MAX_PROBLEMS + 1))
    assert lib.osh_orb_sim3_ransac(None, capi.OSH_SIM3R_MAX_PROBLEMS + 1, cp, cr) == capi.OSH_ERR_UNSUPPORTED
    assert "more than 64 problems" in capi.last_error(lib)
    # the scoring entry refuses the same points, and too many transforms
    T = np.zeros((capi.OSH_SIM3R_MAX_ITERATIONS + 1, 13), np.float32)
    count, mask = np.zeros(len(T), np.int32), np.zeros((len(T), capi.ransac_mask_words(pb.n)), np.uint32)
    cp, cr, _keep, _outs = orb.sim3_ransac_args([pb])
    args = (capi.ptr(T, capi.c_float_p), capi.ptr(count, capi.c_int32_p), capi.ptr(mask, capi.c_uint32_p))
    assert lib.osh_orb_sim3_ransac_check_inliers(None, cp, len(T), *args) == capi.OSH_ERR_UNSUPPORTED and "more than 1024 transforms" in capi.last_error(lib)
    # a valid call passes the validation: all that is missing here is the context
    assert lib.osh_orb_sim3_ransac(None, 1, cp, cr) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
    assert lib.osh_orb_sim3_ransac_check_inliers(None, cp, 2, *args) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
    # no problems, no work, no context needed before that is known
    assert lib.osh_orb_sim3_ransac(None, 0, None, None) == capi.OSH_ERR_INVALID
    # and the host build still answers
    sc.assert_self_consistent(pb, orb.sim3_ransac_cpu([pb], debug=True)[0][0])


def test_ransac_parameters():
    for N, m, mx in ((100, 6, 300), (20, 6, 300), (6, 6, 300), (5, 6, 300), (7, 6, 300), (40, 20, 300), (40, 20, 5), (300, 150, 35), (10, 9, 300)):
        assert orb.sim3_ransac_stage("max_iterations", N, 0.99, m, mx) == s3n.max_iterations(N, 0.99, m, mx), (N, m, mx)
    assert orb.sim3_ransac_stage("max_iterations", 6, 0.99, 6, 300) == 1          # N == minInliers
    assert orb.sim3_ransac_stage("max_iterations", 100, 0.99, 6, 300) == 300      # epsilon^3 is tiny: the cap
    assert orb.sim3_ransac_stage("max_iterations", 40, 0.99, 20, 300) == 35       # ceil(log(0.01) / log(1 - 0.125))
