"""osh_orb_describe and ORBextractor::operator() on the device against the numpy restatement of tests/brief_numpy.py: the blurred
levels and the descriptors as bytes, cos and sin as bit patterns, for every keypoint, without tolerance.  The debug outputs are
compared first, so that a failure names its stage."""
import numpy as np
import pytest

import brief_numpy as bn
import fast_numpy as fn
from orb_slam3_study_kr_amd import capi, orb, synth
from orb_slam3_study_kr_amd import synth_fast as sf

pytestmark = pytest.mark.gpu
F = np.float32


def _check(m, names, what, borders=None):
    got = m.describe([bn.case(n)[0] for n in names], borders=borders, debug=True)
    for k, n in enumerate(names):
        bn.assert_same(got[k], bn.case(n)[1], f"{what}[{k}] {n}")
    return got


@pytest.mark.parametrize("name", bn.CASE_NAMES)
def test_committed_cases_equal_the_restatement(hip_lib, name):
    with orb.OrbMatcher(0) as m:
        for border in (0, 3):
            _check(m, [name], f"border {border}", borders=[border])
        plain = m.describe([bn.case(name)[0]])[0]      # without the debug outputs: only the levels with keypoints are blurred
        bn.assert_same(plain, bn.case(name)[1], f"{name} without debug outputs", debug=False)


@pytest.mark.parametrize("shape", [(16, 64), (16, 128), (32, 64), (17, 65), (4, 4), (4, 300), (300, 4), (15, 63)])
def test_blur_export_around_the_tile(hip_lib, shape):
    """Levels of exactly one tile, exactly two in either direction, one pixel more or less, and the smallest level, blur only."""
    img = bn.noise_level(shape[0] * 7 + shape[1], *shape)
    it = dict(pyramid=(img,), xy=np.zeros((0, 2), F), level=np.zeros(0, np.int32), angle=np.zeros(0, F), pattern=bn.seeded_table(1))
    with orb.OrbMatcher(0) as m:
        for w in (None, [0, 0, 0, 256, 0, 0, 0], [256, 0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6, 235]):
            got = m.describe([dict(it, blur_q8=w)], debug=True)[0]
            assert np.array_equal(got["blurred"][0], bn.blur(img, w)), (shape, w)
            if w is not None and w[3] == 256:
                assert np.array_equal(got["blurred"][0], img)


def test_a_level_too_small_for_the_blur(hip_lib):
    ok = dict(pyramid=(bn.noise_level(1, 4, 4),), xy=np.zeros((0, 2), F), level=np.zeros(0, np.int32), angle=np.zeros(0, F), pattern=bn.seeded_table(1))
    small = dict(ok, pyramid=(bn.noise_level(2, 3, 50),))
    with orb.OrbMatcher(0) as m:
        assert np.array_equal(m.describe([ok], debug=True)[0]["blurred"][0], bn.blur(ok["pyramid"][0]))
        with pytest.raises(capi.OshError) as e:
            m.describe([small], debug=True)
        assert e.value.code == capi.OSH_ERR_UNSUPPORTED and "fewer than 4 rows or columns" in str(e.value)
        assert m.describe([small])[0]["descriptors"].shape == (0, 32)      # without the export the level is skipped
        # a pyramid whose last level is too small, keypoints on the first
        it = bn.item("one_39x39")
        mixed = dict(it, pyramid=it["pyramid"] + (np.zeros((3, 3), np.uint8),))
        bn.assert_same(m.describe([mixed])[0], bn.case("one_39x39")[1], "a small level without keypoints", debug=False)


def test_more_than_2_24_keypoints_are_unsupported(hip_lib):
    """17 frames of 2^20 keypoints that share their arrays: refused after validation, before any device work."""
    n = 1 << 20
    it = dict(pyramid=(np.zeros((39, 39), np.uint8),), xy=np.full((n, 2), 19, F), level=np.zeros(n, np.int32), angle=np.zeros(n, F), pattern=bn.seeded_table(1))
    cf, cr, _keep, _ = orb.describe_args([it])
    frames = (capi.DescribeFrame * 17)(*[cf[0]] * 17)
    results = (capi.DescribeResult * 17)(*[cr[0]] * 17)
    with orb.OrbMatcher(0) as m:
        assert m.lib.osh_orb_describe(m.ctx, 17, frames, results) == capi.OSH_ERR_UNSUPPORTED
        assert "2^24" in capi.last_error(m.lib)
        _check(m, ["one_39x39"], "after the refusal")


def _detect_frame(name):
    it = bn.case(name)[0]
    return sf.FastFrame(it["pyramid"])


def test_by_token_and_by_pyramid(hip_lib):
    a, b = "pyramid_120x90", "tile_65x129"
    shapes = lambda n: [p.shape for p in bn.case(n)[0]["pyramid"]]
    with orb.OrbMatcher(0) as m, orb.OrbMatcher(0) as other:
        first = m.fast_detect([_detect_frame(a), _detect_frame(b)])
        by_token = lambda n, k: bn.item(n, pyramid=None, token=first[k]["token"], shapes=shapes(n))
        got = m.describe([by_token(b, 1), bn.item("extremes_45x52"), by_token(a, 0)], debug=True)
        for g, n in zip(got, (b, "extremes_45x52", a)):
            bn.assert_same(g, bn.case(n)[1], f"{n}: tokens and a pyramid in one call")
        bn.assert_same(m.describe([by_token(a, 0)], debug=True)[0], bn.case(a)[1], "the token outlives describe calls")
        # IC_Angle still reads the resident pyramid after describe calls
        kxy = np.asarray([[30, 30]], F)
        ang = m.ic_angle([dict(xy=kxy, level=np.zeros(1, np.int32), token=first[0]["token"])])[0]
        fn.assert_angles_same(ang, fn.ic_angle(bn.case(a)[0]["pyramid"], kxy, np.zeros(1, np.int32)), "ic_angle by token after describe")
        # keypoints are checked against the resident levels: level 2 of `a` cannot hold what level 0 can
        with pytest.raises(capi.OshError) as e:
            m.describe([dict(by_token(a, 0), xy=np.asarray([[70, 40]], F), level=np.asarray([2], np.int32), angle=np.zeros(1, F))])
        assert e.value.code == capi.OSH_ERR_INVALID and "leaves level 2" in str(e.value)
        # another context's token, and numbers that were never handed out
        other.fast_detect([_detect_frame(b)])
        for bad in (first[0]["token"] + 2, 0, 2 ** 63):
            with pytest.raises(capi.OshError) as e:
                m.describe([dict(by_token(a, 0), token=bad)])
            assert e.value.code == capi.OSH_ERR_INVALID and "token" in str(e.value)
        with pytest.raises(capi.OshError):
            other.describe([by_token(a, 0)])
        # the next detect makes the token stale
        second = m.fast_detect([_detect_frame(b)])
        with pytest.raises(capi.OshError) as e:
            m.describe([by_token(a, 0)])
        assert "token" in str(e.value)
        bn.assert_same(m.describe([bn.item(b, pyramid=None, token=second[0]["token"], shapes=shapes(b))], debug=True)[0], bn.case(b)[1], "the new token")


MIXED = ["pyramid_120x90", "one_39x39", "asymmetric_weights", "reach_22", "tile_50x131"]


def test_batches_equal_single_calls(hip_lib):
    with orb.OrbMatcher(0) as m:
        for names, borders in ((["extremes_45x52"], None), (["identity_weights", "checker"], [2, 0]), (MIXED, [0, 1, 0, 7, 0])):
            batch = _check(m, names, f"batch of {len(names)}", borders=borders)
            for k, n in enumerate(names):
                one = _check(m, [n], f"single {n}")[0]
                assert np.array_equal(one["descriptors"], batch[k]["descriptors"]) and np.array_equal(one["cos_sin"], batch[k]["cos_sin"])


@pytest.fixture()
def zero_new_buffers():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OSH_ZERO_NEW_BUFFERS", "1")
        yield


def test_long_lived_context_equals_fresh_contexts(hip_lib, zero_new_buffers):
    later = [["one_39x39"], ["const_0", "tile_41x70"], MIXED[:3], ["edges_60x70"]]
    pair = synth.make_orb_pair(9, 2000, 2000)
    with orb.OrbMatcher(0) as m:
        m.search([pair])
        _check(m, ["vga_752x480_L8", "tile_65x129"], "warm-up")
        for k, names in enumerate(later):
            got = _check(m, names, f"step {k}")
            m.search([pair], windowed=False)
            with orb.OrbMatcher(0) as fresh:
                ref = _check(fresh, names, f"step {k} fresh")
            for g, r in zip(got, ref):
                assert np.array_equal(g["descriptors"], r["descriptors"])


def test_one_752x480_frame_of_eight_levels(hip_lib):
    with orb.OrbMatcher(0) as m:
        got = _check(m, ["vga_752x480_L8"], "752x480", borders=[19])
    assert got[0]["descriptors"].shape[0] > 1000 and len(got[0]["blurred"]) == 8


def _expected_extract(r, lapping):
    """_keypoints, descriptors and the return value from the restatement applied to what the wrapper returned."""
    n = int(r["level_count"].sum())
    level = np.repeat(np.arange(len(r["level_count"])), r["level_count"]).astype(np.int32)
    exp = bn.describe(r["pyramid"], r["level_xy"], level, r["level_angle"], orb.standin_pattern())
    sfs = np.cumprod(np.concatenate([[F(1)], np.full(len(r["level_count"]) - 1, F(1.2), F)]), dtype=F)
    xy = r["level_xy"].copy()
    up = level > 0
    xy[up] = (xy[up] * sfs[level[up], None]).astype(F)
    order, mono, stereo = np.zeros(n, np.int64), 0, n - 1
    for i in range(n):
        if lapping[0] <= xy[i, 0] <= lapping[1]:
            order[i], stereo = stereo, stereo - 1
        else:
            order[i], mono = mono, mono + 1
    out_xy, out_desc, out_oct, out_ang = np.zeros((n, 2), F), np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.zeros(n, F)
    out_xy[order], out_desc[order], out_oct[order], out_ang[order] = xy, exp["descriptors"], level, r["level_angle"]
    return mono, out_xy, out_desc, out_oct, out_ang


@pytest.mark.parametrize("lapping", [(0, 0), (100, 180), (-5, 10000)])
def test_operator_call_through_the_stand_in(hip_lib, lapping):
    img = sf.make_image(31, 200, 260)
    r = orb.extract(img, nfeatures=300, nlevels=4, lapping=lapping)
    n = int(r["level_count"].sum())
    assert n > 100 and r["n"] == n and r["desc_rows"] == n and (r["level_count"] > 0).sum() >= 3
    assert [p.shape for p in r["pyramid"]] == sf.level_sizes(200, 260, 4) and np.array_equal(r["pyramid"][0], img)
    mono, xy, desc, octave, angle = _expected_extract(r, lapping)
    assert r["ret"] == mono
    if lapping == (100, 180):
        assert 0 < mono < n      # the lapping area splits the keypoints
    elif lapping == (-5, 10000):
        assert mono == 0
    assert np.array_equal(r["xy"].view(np.uint32), xy.view(np.uint32)) and np.array_equal(r["octave"], octave)
    assert np.array_equal(r["angle"].view(np.uint32), angle.view(np.uint32))
    bad = np.argwhere((r["descriptors"] != desc).any(axis=1)).ravel()
    assert not len(bad), f"{len(bad)} of {n} descriptors differ, first {bad[:5]}"


def test_operator_call_without_keypoints(hip_lib):
    r = orb.extract(None, nlevels=3)                                    # an empty image
    assert r["ret"] == -1
    r = orb.extract(np.full((120, 160), 90, np.uint8), nlevels=3)       # no corners: descriptors released
    assert r["ret"] == 0 and r["n"] == 0 and r["desc_rows"] == 0 and r["level_count"].sum() == 0
    r = orb.extract(sf.make_image(5, 120, 160), nfeatures=100, nlevels=3)      # and the thread's context serves the next call
    assert r["n"] > 20 and r["ret"] == r["n"]


def test_time_slots(hip_lib):
    with orb.OrbMatcher(0) as m:
        assert (m.describe_times() == 0).all()
        m.set_profiling(True)
        m.describe([bn.case("tile_41x70")[0]])
        assert (m.describe_times() > 0).all()
