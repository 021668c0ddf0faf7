"""osh_orb_mlpnp_solve (MLPnPsolver::iterate, the PnP RANSAC of relocalisation) on the device: the scoring stage against the numpy
float32 statement, the self-consistency of the full run (counts at the device's own poses, records and first_hit by the Python
restatement of the decision), hypothesis and refine poses against the numpy restatement within the bound of mlpnp_cases.py,
degenerate sets, the end-to-end run against the generator's truth through the entry and the host build, refusals, and the same bits
alone and inside a batch."""
import dataclasses
import functools

import numpy as np
import pytest

import mlpnp_cases as mc
import mlpnp_numpy as mn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_mlpnp as sm

pytestmark = pytest.mark.gpu

SIZES = (10, 11, 63, 64, 65, 300)
NUMPY_VS_TRUTH = mc.NUMPY_VS_TRUTH
end_to_end = mc.end_to_end


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


@functools.lru_cache(maxsize=None)
def problem(n, iterations, camera=sm.PINHOLE, seed=1, plane_z=None, noise=0.5):
    return sm.make_problem(seed=seed + n, n=n, iterations=iterations, camera_type=camera, outlier_share=0.3, noise_px=noise, plane_z=plane_z,
                           min_inliers=6)


def perturbed(pose, rng, scale):
    R = sm.rodrigues(rng.normal(0, scale, 3)) @ pose[:9].reshape(3, 3)
    return np.concatenate([R.reshape(9), pose[9:] + rng.normal(0, scale, 3)])


def numpy_flags(pb, pose):
    return mn.check_inliers(pb.camera_type, pb.camera, pose, pb.p3d, pb.p2d, pb.max_error)


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k}"


def assert_self_consistent(pb, o, what):
    """Counts at the device's own poses (Pinhole: the numpy float32 statement, bit for bit), records, first_hit and the running best
    by the Python restatement of the decision from the device's own counts and refine outcomes; the masks and poses that go with them."""
    n, it = pb.n, pb.sets.shape[0]
    if pb.camera_type == sm.PINHOLE:
        for k in range(it):
            assert int(numpy_flags(pb, o["debug_pose"][k]).sum()) == o["debug_count"][k], f"{what}: count of iteration {k}"
    records, d = mn.replay(o["debug_count"], pb.min_inliers, pb.best_inliers_in, pb.best_refine_ok_in, o["debug_record_count"])
    assert list(o["debug_record"][:len(records)]) == records and np.all(o["debug_record"][len(records):] == -1), what
    assert np.all(o["debug_record_count"][len(records):] == 0) and np.all(o["debug_record_pose"][len(records):] == 0), what
    for k, v in d.items():
        assert int(o[k][0]) == int(v), f"{what}: {k}: {int(o[k][0])} vs {int(v)}"
    hit, best = int(o["hit_record"][0]), int(o["best_iteration"][0])
    if hit >= 0:
        assert np.array_equal(o["hit_pose"].view(np.uint64), o["debug_record_pose"][hit].view(np.uint64)), what
        flags = orb.mask_bits(o["hit_mask"], n)
        assert int(flags.sum()) == int(o["hit_count"][0]), what
        if pb.camera_type == sm.PINHOLE:
            assert np.array_equal(flags, numpy_flags(pb, o["hit_pose"])), what
    else:
        assert not o["hit_pose"].any() and not o["hit_mask"].any() and int(o["hit_count"][0]) == 0, what
    if best >= 0:
        assert np.array_equal(o["best_pose"].view(np.uint64), o["debug_pose"][best].view(np.uint64)), what
        flags = orb.mask_bits(o["best_mask"], n)
        assert int(flags.sum()) == int(o["best_count"][0]) == int(o["debug_count"][best]), what
        if pb.camera_type == sm.PINHOLE:
            assert np.array_equal(flags, numpy_flags(pb, o["best_pose"])), what
    else:
        assert not o["best_pose"].any() and not o["best_mask"].any(), what
    # mask bits beyond n stay 0
    for name in ("hit_mask", "best_mask"):
        assert not orb.mask_bits(o[name], 32 * o[name].shape[0])[n:].any(), what


# ------------------------------------------------------------------------------------------------------------ scoring
@pytest.mark.parametrize("n", SIZES)
def test_scoring_pinhole_equals_numpy_bit_for_bit(matcher, n):
    pb = problem(n, 1)
    rng = np.random.RandomState(n)
    poses = np.stack([pb.pose] + [perturbed(pb.pose, rng, s) for s in (1e-6, 1e-4, 2e-3, 1e-2, 1e-1, 1.0)])
    count, mask = matcher.mlpnp_check_inliers(pb, poses)
    flags = orb.mask_bits(mask, n)
    for k, pose in enumerate(poses):
        want = numpy_flags(pb, pose)
        assert np.array_equal(flags[k], want), f"pose {k}"
        assert count[k] == want.sum()
    assert not orb.mask_bits(mask, 32 * mask.shape[1])[:, n:].any()
    assert 0 < count[3] and count[6] < count[0] == pb.inlier.sum()   # the poses span all-inliers-found to almost none


@pytest.mark.parametrize("n", (65, 300))
def test_scoring_kb8_equals_numpy_away_from_the_threshold(matcher, n):
    pb = sm.make_problem(seed=40 + n, n=n, iterations=1, camera_type=sm.KB8, outlier_share=0.5, noise_px=0.5)
    rng = np.random.RandomState(n)
    poses = np.stack([pb.pose] + [perturbed(pb.pose, rng, 1e-5) for _ in range(4)])
    want = []
    for pose in poses:
        flags, e2 = mn.check_inliers(pb.camera_type, pb.camera, pose, pb.p3d, pb.p2d, pb.max_error, with_error=True)
        assert np.all(np.abs(e2.astype(np.float64) - pb.max_error) > 1e-3 * pb.max_error), "a point lies near its threshold"
        want.append(flags)
    count, mask = matcher.mlpnp_check_inliers(pb, poses)
    assert np.array_equal(orb.mask_bits(mask, n), np.stack(want))
    assert np.array_equal(count, np.stack(want).sum(1))
    assert np.array_equal(want[0], pb.inlier)


# ------------------------------------------------------------------------------------------------------------ the full run
@pytest.mark.parametrize("n,iterations", [(10, 1), (11, 3), (63, 3), (64, 300), (65, 3), (300, 300)])
def test_full_run_is_self_consistent(matcher, n, iterations):
    pb = problem(n, iterations)
    o = matcher.mlpnp_solve([pb], debug=True, fill=0xCD)[0]
    assert_self_consistent(pb, o, f"n {n}, {iterations} iterations")


def test_batch_of_unequal_problems_and_a_running_best_on_entry(matcher):
    """Five problems of unequal N and iteration counts, both cameras, the z = 0 plane, an empty problem, and a best on entry (with a
    successful and with a failed Refine) in one call: every one as when it runs alone."""
    pbs = [problem(300, 300), problem(65, 3, sm.KB8), problem(64, 7, plane_z=0.0), dataclasses.replace(problem(63, 40), best_inliers_in=30, best_refine_ok_in=1),
           problem(11, 0), dataclasses.replace(problem(300, 300, sm.KB8), best_inliers_in=150, best_refine_ok_in=0)]
    outs = matcher.mlpnp_solve(pbs, debug=True, fill=0xCD)
    for k, (pb, o) in enumerate(zip(pbs, outs)):
        assert_self_consistent(pb, o, f"problem {k}")
        assert_same(matcher.mlpnp_solve([pb], debug=True)[0], o, f"problem {k} alone")
    assert int(outs[0]["first_hit"][0]) >= 0 and int(outs[0]["n_records"][0]) >= 1
    # the best on entry with a successful Refine: the first iteration with enough inliers is the hit, with no record of this call
    hit = int(outs[3]["first_hit"][0])
    assert hit >= 0 and outs[3]["debug_count"][hit] >= pbs[3].min_inliers and np.all(outs[3]["debug_count"][:hit] < pbs[3].min_inliers)
    assert int(outs[4]["first_hit"][0]) == -1 and int(outs[4]["best_count"][0]) == 0


def test_same_bits_alone_and_as_problem_3_of_5(matcher):
    pb = end_to_end(sm.PINHOLE, 0.5)
    alone = matcher.mlpnp_solve([pb], debug=True)[0]
    batch = matcher.mlpnp_solve([problem(65, 3), problem(300, 300, sm.KB8), pb, problem(11, 3), problem(64, 300)], debug=True, fill=0xEE)
    assert_same(alone, batch[2], "problem 3 of 5")


# ------------------------------------------------------------------------------------------------------------ poses against numpy
def test_hypothesis_poses_meet_the_measured_bound(matcher):
    """The minimal sets of mlpnp_cases.pose_cases() (drawn from the inliers only): the device's pose of every iteration against the
    numpy restatement, within 4 x the host build's own spread."""
    kinds = ("pinhole", "kb8", "planar")
    outs = matcher.mlpnp_solve([mc.scene(k) for k in kinds], debug=True)
    poses = []
    seen = {k: 0 for k in kinds}
    for kind, group, idx, ref in mc.pose_cases():
        if len(idx) == 6:
            poses.append(outs[kinds.index(kind)]["debug_pose"][seen[kind]])
            seen[kind] += 1
        else:
            poses.append(ref)   # the refine case: test_refine_pose_meets_the_measured_bound
    for group in ("general", "planar"):
        rot, trans = mc.spread(poses, group)
        print(f"{group}: device vs numpy: rotation {rot:.3e} rad, translation {trans:.3e}; bound {mc.DEVICE_BOUND[group]}")
        assert rot <= mc.DEVICE_BOUND[group][0] and trans <= mc.DEVICE_BOUND[group][1], group


@pytest.mark.parametrize("kind", ("pinhole", "kb8"))
def test_refine_pose_meets_the_measured_bound(matcher, kind):
    """The refined pose at the hit against numpy's computePose over the same inliers (the best mask); in these scenes the best mask
    is the true inlier set."""
    pb = mc.scene(kind)
    o = matcher.mlpnp_solve([pb], debug=True)[0]
    assert int(o["first_hit"][0]) >= 0 and int(o["hit_record"][0]) >= 0
    flags = orb.mask_bits(o["best_mask"], pb.n)
    assert np.array_equal(flags, pb.inlier)
    idx = np.flatnonzero(flags)
    rot, trans = mn.pose_difference(o["hit_pose"], mn.compute_pose(pb.bearing[idx], pb.p3d[idx]))
    print(f"{kind}: refine, device vs numpy: rotation {rot:.3e} rad, translation {trans:.3e}; bound {mc.DEVICE_BOUND['general']}")
    assert rot <= mc.DEVICE_BOUND["general"][0] and trans <= mc.DEVICE_BOUND["general"][1]


# ------------------------------------------------------------------------------------------------------------ degenerate sets
def test_degenerate_sets_return_and_leave_their_neighbours_alone(matcher):
    base = problem(65, 3)
    healthy = problem(64, 300)
    # a repeated point: correspondence 1 is a copy of correspondence 0, both in the set
    rep = dataclasses.replace(base, bearing=base.bearing.copy(), p3d=base.p3d.copy(), p2d=base.p2d.copy(), sets=base.sets.copy())
    rep.bearing[1], rep.p3d[1], rep.p2d[1] = rep.bearing[0], rep.p3d[0], rep.p2d[0]
    rep.sets[0] = [0, 1, 2, 3, 4, 5]
    # all six on one ray through the camera centre
    ray = dataclasses.replace(base, bearing=base.bearing.copy(), p3d=base.p3d.copy(), sets=base.sets.copy())
    R, t = base.pose[:9].reshape(3, 3), base.pose[9:]
    centre, direction = -R.T @ t, R.T @ base.bearing[0]
    for j in range(6):
        ray.p3d[j] = (centre + (3.0 + j) * direction).astype(np.float32)
        ray.bearing[j] = base.bearing[0]
    ray.sets[:] = [0, 1, 2, 3, 4, 5]
    # a NaN coordinate in a correspondence of every set
    nan = dataclasses.replace(base, p3d=base.p3d.copy(), sets=base.sets.copy())
    nan.p3d[7, 1] = np.nan
    nan.sets[:, 0] = 7
    nan.sets[:, 1:] = [[1, 2, 3, 4, 5], [8, 9, 10, 11, 12], [13, 14, 15, 16, 17]]
    alone = matcher.mlpnp_solve([healthy], debug=True)[0]
    outs = matcher.mlpnp_solve([rep, healthy, ray, nan], debug=True, fill=0xCD)
    assert_same(alone, outs[1], "the healthy neighbour")
    fill32, fill64 = np.uint32(0xCDCDCDCD), np.uint64(0xCDCDCDCDCDCDCDCD)
    for name, pb, o in (("repeated point", rep, outs[0]), ("one ray", ray, outs[2]), ("NaN", nan, outs[3])):
        for k, v in o.items():
            bits = v.view(np.uint64 if v.dtype.itemsize == 8 else np.uint32)
            assert not np.any(bits == (fill64 if v.dtype.itemsize == 8 else fill32)), f"{name}: {k} not written"
        for k in range(pb.sets.shape[0]):
            pose = o["debug_pose"][k]
            want = int(numpy_flags(pb, pose).sum()) if np.all(np.isfinite(pose)) else 0
            assert o["debug_count"][k] == want, f"{name}: iteration {k}"
        assert_self_consistent(pb, o, name)
    assert np.all(outs[3]["debug_count"] == 0) and int(outs[3]["first_hit"][0]) == -1


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("camera", (sm.PINHOLE, sm.KB8))
@pytest.mark.parametrize("noise", (0.0, 0.5))
def test_end_to_end_against_the_truth(matcher, camera, noise):
    """300 points, 50 % outliers, through the entry and through the host build: a hit, every true inlier flagged and no outlier, and
    the refined pose against the generator's truth."""
    pb = end_to_end(camera, noise)
    bound = mc.DEVICE_BOUND["general"] if noise == 0.0 else tuple(2 * v for v in NUMPY_VS_TRUTH[camera])
    for name, o in (("device", matcher.mlpnp_solve([pb])[0]), ("host build", orb.mlpnp_cpu([pb])[0][0])):
        assert int(o["first_hit"][0]) >= 0 and int(o["best_refine_ok"][0]) == 1, name
        assert np.array_equal(orb.mask_bits(o["hit_mask"], pb.n), pb.inlier), name
        assert int(o["hit_count"][0]) == pb.inlier.sum() > pb.min_inliers
        rot, trans = mn.pose_difference(o["hit_pose"], pb.pose)
        print(f"{name}, camera {camera}, noise {noise}: against truth: rotation {rot:.3e} rad, translation {trans:.3e}; bound {bound}")
        assert rot <= bound[0] and trans <= bound[1], name


def test_device_and_host_build_take_the_same_decisions(matcher):
    pbs = [end_to_end(sm.PINHOLE, 0.5), end_to_end(sm.KB8, 0.5), problem(65, 3), problem(64, 300)]
    dev = matcher.mlpnp_solve(pbs, debug=True)
    cpu = orb.mlpnp_cpu(pbs, debug=True)[0]
    for k, (a, b) in enumerate(zip(dev, cpu)):
        for name in ("first_hit", "hit_record", "hit_count", "best_iteration", "best_count", "best_refine_ok", "n_records", "hit_mask", "best_mask"):
            assert np.array_equal(a[name], b[name]), f"problem {k}: {name}"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(matcher):
    pb = problem(65, 3)
    before = matcher.mlpnp_solve([pb], debug=True)[0]
    sets = pb.sets.copy(); sets[1, 5] = sets[1, 2]
    out_of_range = pb.sets.copy(); out_of_range[2, 0] = pb.n
    bad = [(dataclasses.replace(pb, sets=sets), "repeats index", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, sets=out_of_range), "outside", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, min_inliers=5), "min_inliers", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, camera_type=2), "camera type", capi.OSH_ERR_INVALID),
           (sm.make_problem(seed=2, n=capi.OSH_MLPNP_MAX_POINTS + 1, iterations=1), "more than 2048 correspondences", capi.OSH_ERR_UNSUPPORTED),
           (dataclasses.replace(pb, sets=np.tile(pb.sets, (342, 1))), "more than 1024 iterations", capi.OSH_ERR_UNSUPPORTED)]
    for problem_, message, code in bad:
        with pytest.raises(capi.OshError, match=message) as err:
            matcher.mlpnp_solve([pb, problem_])
        assert err.value.code == code
        assert_same(matcher.mlpnp_solve([pb], debug=True)[0], before, f"after '{message}'")
    with pytest.raises(capi.OshError, match="more than 64 problems") as err:
        matcher.mlpnp_solve([pb] * (capi.OSH_MLPNP_MAX_PROBLEMS + 1))
    assert err.value.code == capi.OSH_ERR_UNSUPPORTED
    assert len(matcher.mlpnp_solve([pb] * capi.OSH_MLPNP_MAX_PROBLEMS)) == capi.OSH_MLPNP_MAX_PROBLEMS
    assert_same(matcher.mlpnp_solve([pb], debug=True)[0], before, "after the refusals")


def test_largest_problem_the_entry_accepts(matcher):
    pb = sm.make_problem(seed=9, n=capi.OSH_MLPNP_MAX_POINTS, iterations=8, inlier_sets=True)
    o = matcher.mlpnp_solve([pb], debug=True, fill=0xCD)[0]
    assert_self_consistent(pb, o, "2048 correspondences")
    assert int(o["first_hit"][0]) >= 0
    assert np.array_equal(orb.mask_bits(o["hit_mask"], pb.n), pb.inlier)
