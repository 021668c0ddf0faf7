"""osh_orb_sim3_ransac on the device against the host build of the same header bit for bit, over the size, iteration, camera and scale
grids; the scoring entry against numpy bit for bit for Pinhole pairs; self-consistency of the full run by the Python scan from the
device's own counts; mask bits beyond n; degenerate sets and a NaN; the end-to-end scenes against the generator's truth; the same
bits alone and at positions 0, 1 and 63 of a batch of 64; refusals that leave the context usable; the largest problem."""
import dataclasses

import numpy as np
import pytest

import sim3_ransac_cases as sc
import sim3_ransac_numpy as s3n
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_sim3_ransac as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


def assert_same(a, b, what, nan_payload=True):
    """Bit for bit; nan_payload=False: a NaN equals a NaN whatever its sign and payload bits (0 / 0 sets the sign bit on x86-64 and
    clears it on the device), everything else still bit for bit."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if not nan_payload and x.dtype == np.float32:
            assert np.array_equal(np.isnan(x), np.isnan(y)), f"{what}: {k}"
            x, y = np.where(np.isnan(x), np.float32(0), x), np.where(np.isnan(y), np.float32(0), y)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {k}"


# ------------------------------------------------------------------------------------------------------------ device == host build
@pytest.mark.parametrize("fix_scale", (True, False))
@pytest.mark.parametrize("cameras", tuple(sc.CAMERAS))
def test_every_array_equals_the_host_build(matcher, cameras, fix_scale):
    pbs = [sc.grid_problem(n, it, cameras, fix_scale) for n in sc.SIZES for it in sc.ITERATIONS]
    host = orb.sim3_ransac_cpu(pbs, debug=True)[0]
    for k in range(0, len(pbs), 6):   # the grid in three calls of six problems, and every problem of the first call alone
        dev = matcher.sim3_ransac(pbs[k:k + 6], debug=True, fill=0xCD)
        for j, o in enumerate(dev):
            assert_same(o, host[k + j], f"n {pbs[k + j].n}, {len(pbs[k + j].sets)} iterations")
    for k in range(6):
        assert_same(matcher.sim3_ransac([pbs[k]], debug=True, fill=0xCD)[0], host[k], f"problem {k} alone")


# ------------------------------------------------------------------------------------------------------------ scoring
@pytest.mark.parametrize("n", sc.SIZES)
def test_scoring_pinhole_equals_numpy_bit_for_bit(matcher, n):
    pb = sc.grid_problem(n, 1, "pinhole-pinhole", False)
    Ts = sc.transforms(pb, n)
    count, mask = matcher.sim3_ransac_check_inliers(pb, Ts)
    flags, clean = sc.mask_bits(mask, n)
    assert clean
    for k, T in enumerate(Ts):
        want, c = s3n.check_inliers(pb, T)
        assert np.array_equal(flags[k], want) and count[k] == c, f"transform {k}"
    assert count[0] == pb.inlier.sum() and count[-1] < max(count[0], 1)


# ------------------------------------------------------------------------------------------------------------ the full run
@pytest.mark.parametrize("n,iterations", [(3, 1), (4, 3), (63, 3), (64, 300), (65, 3), (300, 300)])
def test_full_run_is_self_consistent(matcher, n, iterations):
    pb = sc.grid_problem(n, iterations, "pinhole-pinhole", False)
    o = matcher.sim3_ransac([pb], debug=True, fill=0xCD)[0]
    sc.assert_self_consistent(pb, o)
    for k in range(min(iterations, 8)):   # the counts at the device's own transforms: the numpy float32 statement
        assert s3n.check_inliers(pb, o["debug_T"][k])[1] == o["debug_count"][k]
    # a best on entry: nothing below it is a record
    pb2 = dataclasses.replace(pb, best_inliers_in=int(o["debug_count"].max()))
    o2 = matcher.sim3_ransac([pb2], debug=True, fill=0xCD)[0]
    sc.assert_self_consistent(pb2, o2)
    assert (o2["record_count"][:int(o2["n_records"][0])] == pb2.best_inliers_in).all()
    # nothing passed but the head: the call still runs
    cp, cr, _keep, outs = orb.sim3_ransac_args([pb])
    for name in ("record", "record_count", "record_T", "record_mask", "debug_count"):
        setattr(cr[0], name, None)
    capi.check(matcher.lib.osh_orb_sim3_ransac(matcher.ctx, 1, cp, cr), "osh_orb_sim3_ransac", matcher.lib)
    assert int(outs[0]["first_hit"][0]) == int(o["first_hit"][0]) and int(outs[0]["n_records"][0]) == int(o["n_records"][0])


@pytest.mark.parametrize("kind", ("collinear", "coincident", "zero_den", "nan"))
def test_degenerate_sets_and_a_nan(matcher, kind):
    pb = sc.grid_problem(65, 3, "pinhole-pinhole", False)
    if kind == "nan":
        x = pb.x3dc2.copy(); x[pb.sets[1, 0], 1] = np.nan
        pb = dataclasses.replace(pb, x3dc2=x)
    else:
        pb = ss.with_degenerate_set(pb, kind)
    o = matcher.sim3_ransac([pb], debug=True, fill=0xCD)[0]
    sc.assert_self_consistent(pb, o)
    assert_same(o, orb.sim3_ransac_cpu([pb], debug=True)[0][0], kind, nan_payload=False)
    if kind == "zero_den":
        assert o["debug_count"][0] == 0 and not np.isfinite(o["debug_T"][0, 12])
    if kind == "nan":
        assert o["debug_count"][1] == 0
    else:
        assert np.isfinite(o["debug_T"][0, :9]).all()


@pytest.mark.parametrize("fix_scale", (True, False))
@pytest.mark.parametrize("seed", sc.END_TO_END_SEEDS)
def test_end_to_end_against_the_truth(matcher, seed, fix_scale):
    pb = sc.end_to_end(seed, fix_scale)
    o = matcher.sim3_ransac([pb], debug=True, fill=0xCD)[0]
    hit = int(o["first_hit"][0])
    assert hit >= 0 and o["debug_count"][hit] > pb.min_inliers
    q = list(o["record"]).index(hit)
    d = sc.truth_difference(pb, o["record_T"][q])
    assert all(a <= b for a, b in zip(d, sc.TRUTH_BOUND)), d
    assert not (sc.mask_bits(o["record_mask"], pb.n)[0][q] & ~pb.inlier).any()


def test_hypotheses_meet_the_measured_bound(matcher):
    for pb, ref in sc.hypothesis_cases():
        o = matcher.sim3_ransac([pb], debug=True)[0]
        assert sc.hypothesis_difference(o["debug_T"], ref) <= sc.HYPOTHESIS_BOUND


def test_same_bits_alone_and_at_positions_0_1_and_63_of_a_batch_of_64(matcher):
    pb = sc.end_to_end(1, False)
    alone = matcher.sim3_ransac([pb], debug=True)[0]
    others = [sc.grid_problem(n, it, cam, fix) for n in sc.SIZES for it in (1, 3) for cam in ("pinhole-pinhole", "kb8-kb8", "pinhole-kb8")
              for fix in (True, False)]
    for pos in (0, 1, 63):
        batch = (others * 2)[:63]
        batch.insert(pos, pb)
        outs = matcher.sim3_ransac(batch, debug=True, fill=0xEE)
        assert len(outs) == 64
        assert_same(alone, outs[pos], f"position {pos}")
    # an empty problem and one without iterations among others
    empty = dataclasses.replace(sc.grid_problem(3, 1, "pinhole-pinhole", True), x3dc1=np.zeros((0, 3), np.float32), x3dc2=np.zeros((0, 3), np.float32),
                                p1im1=np.zeros((0, 2), np.float32), p2im2=np.zeros((0, 2), np.float32), max_error1=np.zeros(0, np.float32),
                                max_error2=np.zeros(0, np.float32), sets=np.zeros((0, 3), np.int32))
    idle = dataclasses.replace(sc.grid_problem(65, 3, "pinhole-pinhole", True), sets=np.zeros((0, 3), np.int32), best_inliers_in=4)
    outs = matcher.sim3_ransac([empty, pb, idle], debug=True, fill=0xEE)
    assert_same(alone, outs[1], "between an empty and an idle problem")
    for o, best in ((outs[0], 0), (outs[2], 4)):
        assert (int(o["first_hit"][0]), int(o["n_records"][0]), int(o["best_iteration"][0]), int(o["best_count"][0])) == (-1, 0, -1, best)


# ------------------------------------------------------------------------------------------------------------ refusals, limits
def test_refusals_leave_the_context_usable(matcher):
    pb = sc.grid_problem(65, 3, "pinhole-pinhole", False)
    before = matcher.sim3_ransac([pb], debug=True)[0]
    repeats = pb.sets.copy(); repeats[1, 2] = repeats[1, 0]
    outside = pb.sets.copy(); outside[2, 0] = pb.n
    bad = [(dataclasses.replace(pb, sets=repeats), "repeats index", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, sets=outside), "outside", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, camera_type2=2), "camera type", capi.OSH_ERR_INVALID),
           (ss.make_problem(seed=2, n=capi.OSH_SIM3R_MAX_POINTS + 1, iterations=1), "more than 4096 correspondences", capi.OSH_ERR_UNSUPPORTED),
           (dataclasses.replace(pb, sets=np.tile(pb.sets, (342, 1))), "more than 1024 iterations", capi.OSH_ERR_UNSUPPORTED)]
    for problem, message, code in bad:
        with pytest.raises(capi.OshError, match=message) as err:
            matcher.sim3_ransac([pb, problem])
        assert err.value.code == code
        assert_same(matcher.sim3_ransac([pb], debug=True)[0], before, f"after '{message}'")
    with pytest.raises(capi.OshError, match="more than 64 problems") as err:
        matcher.sim3_ransac([pb] * (capi.OSH_SIM3R_MAX_PROBLEMS + 1))
    assert err.value.code == capi.OSH_ERR_UNSUPPORTED
    assert_same(matcher.sim3_ransac([pb], debug=True)[0], before, "after the refusals")


def test_largest_problem_the_entry_accepts(matcher):
    pb = ss.make_problem(seed=9, n=capi.OSH_SIM3R_MAX_POINTS, iterations=capi.OSH_SIM3R_MAX_ITERATIONS, fix_scale=False, min_inliers=1000)
    o = matcher.sim3_ransac([pb], debug=True, fill=0xCD)[0]
    sc.assert_self_consistent(pb, o)
    assert_same(o, orb.sim3_ransac_cpu([pb], debug=True)[0][0], "4096 correspondences, 1024 iterations")


def test_times_are_reported_under_profiling(matcher):
    pb = sc.grid_problem(300, 300, "pinhole-pinhole", False)
    matcher.set_profiling(True)
    try:
        matcher.sim3_ransac([pb])
        ms = matcher.sim3_ransac_times()
    finally:
        matcher.set_profiling(False)
    assert (ms > 0).all() and ms.sum() < 1000
