"""A rectified stereo frame extracted and matched on the device: osh_orb_stereo_match_resident (the stereo stage on resident
pyramids), osh_orb_extract_stereo (the fused call) and Frame::ExtractAndMatchStereo, bit for bit against the chain of the entries
that were there before them: osh_orb_extract / osh_orb_extract_raw with the levels downloaded, the level-0 scaling on the host and
osh_orb_stereo_match on those keypoints and levels; the stereo fields also against tests/stereo_numpy.py."""
import dataclasses
import functools

import numpy as np
import pytest

import stereo_frame_cases as sc
import stereo_numpy as sn
from orb_slam3_study_kr_amd import capi, host, orb
from orb_slam3_study_kr_amd import synth_stereo as ss
from orb_slam3_study_kr_amd import synth_stereo_pair as sp

pytestmark = pytest.mark.gpu
F = np.float32
EXTRACT_FIELDS = ("level_count", "xy", "level", "response", "angle", "size", "descriptors")


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


def _same_extract(got, exp, what):
    assert got["n_out"] == exp["n_out"], f"{what}: {got['n_out']} keypoints, {exp['n_out']} expected"
    for k in EXTRACT_FIELDS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, f"{what}: {k} shape {g.shape} != {e.shape}"
        if g.dtype == np.float32:
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(g, e), f"{what}: {k} differs at {np.argwhere(g != e)[:5].tolist()}"


def _chain(m, p, raw=False):
    """The entries that were there before: both images extracted with the levels downloaded, the keypoints scaled on the host, the
    stereo stage on what came down.  Returns the two extract results, the frame and the stereo result."""
    ex = (m.extract_raw if raw else m.extract)([p["left"], p["right"]], download=True)
    fr = sc.stereo_frame(p, ex[0], ex[1], ex[0]["levels"], ex[1]["levels"])
    return ex, fr, m.stereo_match([fr], stages=True)[0]


@functools.lru_cache(maxsize=None)
def _expected(name, raw=False):
    with orb.OrbMatcher(0) as m:
        return _chain(m, sc.pair(name), raw)


@functools.lru_cache(maxsize=None)
def _numpy(name):
    return sn.compute_stereo_matches(_expected(name)[1])


def _same_pair(got, exp, what):
    ex, _fr, st = exp
    _same_extract(got["left"], ex[0], f"{what} left")
    _same_extract(got["right"], ex[1], f"{what} right")
    assert got["stereo"] is not None, what
    sn.assert_same(got["stereo"], st, what=what)


# ---------------------------------------------------------------------------------------------- 1. the stage on resident pyramids
def _resident_against_brought(m, fr, what):
    """fr brings keypoints and the two level-0 images; both pyramids are built on the device, downloaded for the yardstick."""
    built = m.pyramid_build([dict(image=fr.left_pyramid[0], inv_scale=fr.inv_scale_factors), dict(image=fr.right_pyramid[0], inv_scale=fr.inv_scale_factors)])
    down = dataclasses.replace(fr, left_pyramid=[np.ascontiguousarray(lv) for lv in built[0]["levels"]],
                               right_pyramid=[np.ascontiguousarray(lv) for lv in built[1]["levels"]])
    got = m.stereo_match_resident([fr], [(built[0]["token"], built[1]["token"])], stages=True)[0]
    exp = m.stereo_match([down], stages=True)[0]
    sn.assert_same(got, exp, what=what)
    again = m.stereo_match_resident([fr], [(built[0]["token"], built[1]["token"])], stages=True)[0]  # the pyramid is only read
    sn.assert_same(again, exp, what=f"{what} again")
    return got


@pytest.mark.parametrize("case", ("seed1", "sparse", "edge_guard"))
def test_resident_stage_on_the_committed_keypoints(matcher, case):
    fr = ss.make_stereo_frame(**dict(sn.CASES)[case])
    got = _resident_against_brought(matcher, fr, case)
    assert (got["stage"] == capi.OSH_STEREO_ACCEPTED).any()


@pytest.mark.parametrize("size,nlevels,nfeatures", (("pair_160x120_L3", 1, 300), ("pair_160x120_L3", 3, 300), ("pair_752x480_L8", 8, 1000)))
def test_resident_stage_on_extracted_keypoints(matcher, size, nlevels, nfeatures):
    named = sp.named_pair(size)
    p = sc.custom_pair(named["left"], named["right"], nlevels, nfeatures)
    ex = matcher.extract([p["left"], p["right"]])
    fr = sc.stereo_frame(p, ex[0], ex[1], [p["left"]["image"]] * nlevels, [p["right"]["image"]] * nlevels)   # level 0 is what is read of them
    got = _resident_against_brought(matcher, fr, f"{size} L{nlevels}")
    assert (got["stage"] == capi.OSH_STEREO_ACCEPTED).sum() * 4 >= len(got["stage"])
    # the tokens of the extract name the same levels: by them the stage gives the same
    ex = matcher.extract([p["left"], p["right"]])
    by_extract = matcher.stereo_match_resident([fr], [(ex[0]["token"], ex[1]["token"])], stages=True)[0]
    sn.assert_same(by_extract, got, what=f"{size} L{nlevels} by the tokens of extract")


def test_resident_stage_in_a_batch_with_swapped_sides(matcher):
    """Two frames of one call on the same resident pair, the second with left and right swapped: every frame reads its own levels."""
    p = sc.pair("pair_240x180_L4")
    ex = matcher.extract([p["left"], p["right"]], download=True)
    a = sc.stereo_frame(p, ex[0], ex[1], ex[0]["levels"], ex[1]["levels"])
    q = dict(p, left=p["right"], right=p["left"])
    b = sc.stereo_frame(q, ex[1], ex[0], ex[1]["levels"], ex[0]["levels"])
    tl, tr = ex[0]["token"], ex[1]["token"]
    got = matcher.stereo_match_resident([a, b], [(tl, tr), (tr, tl)], stages=True)
    exp = matcher.stereo_match([a, b], stages=True)
    for k in range(2):
        sn.assert_same(got[k], exp[k], what=f"frame {k}")


# ---------------------------------------------------------------------------------------------- 2. the fused call equals the chain
@pytest.mark.parametrize("raw", (False, True), ids=("grey", "raw"))
@pytest.mark.parametrize("name", sc.PAIR_NAMES)
def test_the_fused_call_equals_the_chain(matcher, name, raw):
    exp = _expected(name, raw)
    got = matcher.extract_stereo([sc.pair(name)], stages=True, raw=raw)[0]
    _same_pair(got, exp, name)
    sn.assert_same(got["stereo"], _numpy(name), what=f"{name} against numpy")
    sc.assert_census(got["stereo"]["stage"], got["left"]["level"], name)
    assert "bordered" not in got["left"]                                              # no pyramid came down
    if name == "pair_752x480_L8":
        assert 900 < got["left"]["n_out"] < 1100 and 900 < got["right"]["n_out"] < 1100


def test_the_fused_call_downloads_the_levels_only_when_asked(matcher):
    name = "pair_160x120_L3"
    ex = _expected(name)[0]
    got = matcher.extract_stereo([sc.pair(name)], stages=True, download=True)[0]
    _same_pair(got, _expected(name), name)
    for side, e in zip(("left", "right"), ex):
        for l, (g, b) in enumerate(zip(got[side]["bordered"], e["bordered"])):
            assert np.array_equal(g, b), f"{side} bordered level {l}"


def test_u_right_and_depth_alone(matcher):
    """The stage outputs may be NULL: mvuRight and mvDepth are the same."""
    name = "pair_240x180_L4"
    got = matcher.extract_stereo([sc.pair(name)])[0]
    assert set(got["stereo"]) == {"u_right", "depth"}
    sn.assert_same(got["stereo"], _expected(name)[2], keys=("u_right", "depth"), what=name)


# ---------------------------------------------------------------------------------------------- 3. shapes where the tail can go wrong
def test_a_uniform_right_image_leaves_every_left_keypoint_without_candidate(matcher):
    left = sp.named_pair("pair_160x120_L3")["left"]
    p = sc.custom_pair(left, np.full_like(left, 113), 3, 300)
    got = matcher.extract_stereo([p], stages=True)[0]
    assert got["right"]["n_out"] == 0 and got["left"]["n_out"] > 50
    st = got["stereo"]
    assert (st["stage"] == capi.OSH_STEREO_NO_CANDIDATE).all() and (st["u_right"] == -1).all() and (st["depth"] == -1).all()
    assert (st["best_right"] == -1).all() and (st["hamming"] == -1).all() and (st["sad"] == -1).all() and (st["best_inc"] == capi.OSH_STEREO_NO_INC).all()
    _same_pair(got, _chain(matcher, p), "uniform right")


def test_a_uniform_left_image_has_nothing_to_match(matcher):
    right = sp.named_pair("pair_160x120_L3")["right"]
    p = sc.custom_pair(np.full_like(right, 113), right, 3, 300)
    got = matcher.extract_stereo([p], stages=True)[0]
    assert got["left"]["n_out"] == 0 and got["right"]["n_out"] > 50
    assert all(len(v) == 0 for v in got["stereo"].values())
    _same_extract(got["right"], matcher.extract([p["right"]])[0], "uniform left, right frame")
    both = sc.custom_pair(np.full_like(right, 113), np.full_like(right, 90), 3, 300)   # no keypoint at all: no tail runs
    got = matcher.extract_stereo([both], stages=True)[0]
    assert got["left"]["n_out"] == 0 and got["right"]["n_out"] == 0 and len(got["stereo"]["stage"]) == 0


def _small_pair():
    left, right = sp.make_pair(17, 67, 67, disparities=(3,), density=3.0, flat_band=False, weak_band=False)
    return sc.custom_pair(left, right, 4, 100)


def test_a_pair_with_keypoints_on_level_0_only(matcher):
    p = _small_pair()
    got = matcher.extract_stereo([p], stages=True)[0]
    assert got["left"]["level_count"][0] > 0 and not got["left"]["level_count"][1:].any()   # the levels above have no cells
    _same_pair(got, _chain(matcher, p), "67x67 L4")


def test_a_batch_of_three_unequal_pairs_equals_the_single_calls(matcher):
    pairs = [sc.pair("pair_240x180_L4"), _small_pair(), sc.pair("pair_160x120_L3")]
    singles = [_chain(matcher, p) for p in pairs]
    batch = matcher.extract_stereo(pairs, stages=True)
    assert len({b[side]["token"] for b in batch for side in ("left", "right")}) == 6
    for k, (got, exp) in enumerate(zip(batch, singles)):
        _same_pair(got, exp, f"pair {k} of the batch")
    raw = matcher.extract_stereo(pairs, stages=True, raw=True)
    for k, (got, exp) in enumerate(zip(raw, singles)):
        _same_pair(got, exp, f"pair {k} of the raw batch")


@pytest.mark.parametrize("short", ("left", "right"))
def test_a_frame_that_does_not_fit_gets_its_counts_and_the_pair_no_stereo_arrays(matcher, short):
    name = "pair_160x120_L3"
    ex, _fr, _st = _expected(name)
    pairs = [sc.pair(name), sc.pair("pair_240x180_L4")]
    ex2 = _expected("pair_240x180_L4")[0]
    caps = [ex[0]["n_out"], ex[1]["n_out"], ex2[0]["n_out"], ex2[1]["n_out"]]
    caps[0 if short == "left" else 1] -= 1
    got = matcher.extract_stereo(pairs, capacities=caps, stages=True)                  # OSH_OK: it did not raise
    small, fits = got[0][short], got[0]["right" if short == "left" else "left"]
    assert small["n_out"] == ex[0 if short == "left" else 1]["n_out"] and small["xy"] is None
    assert np.array_equal(small["level_count"], ex[0 if short == "left" else 1]["level_count"])
    _same_extract(fits, ex[1 if short == "left" else 0], "the frame that fits")
    assert got[0]["stereo"] is None
    for k, v in got[0]["stereo_arrays"].items():
        assert not v.any(), f"{k} of the pair was written"
    _same_pair(got[1], _expected("pair_240x180_L4"), "the other pair of the call")
    again = matcher.extract_stereo(pairs, stages=True)                                 # sized by a first call
    _same_pair(again[0], _expected(name), "the repeated call")


# ---------------------------------------------------------------------------------------------- 4. tokens and state
def test_tokens_that_name_nothing_are_refused_and_the_pyramid_stays(matcher):
    p = sc.pair("pair_160x120_L3")
    ex, fr, st = _expected("pair_160x120_L3")
    items = [dict(image=p["left"]["image"], inv_scale=p["left"]["inv_scale"]), dict(image=p["right"]["image"], inv_scale=p["right"]["inv_scale"])]
    old = matcher.pyramid_build(items, download=False)
    new = matcher.pyramid_build(items, download=False)
    good = (new[0]["token"], new[1]["token"])
    with pytest.raises(capi.OshError, match="frame 0: the token names no frame of this context's resident pyramid") as e:
        matcher.stereo_match_resident([fr], [(old[0]["token"], new[1]["token"])], stages=True)            # stale
    assert e.value.code == capi.OSH_ERR_INVALID
    sn.assert_same(matcher.stereo_match_resident([fr], [good], stages=True)[0], st, what="after the stale token")
    with orb.OrbMatcher(0) as other:
        theirs = other.pyramid_build(items, download=False)
        with pytest.raises(capi.OshError, match="names no frame of this context's resident pyramid"):
            matcher.stereo_match_resident([fr], [(theirs[0]["token"], theirs[1]["token"])])                 # of another context
        with pytest.raises(capi.OshError, match="names no frame"):
            other.stereo_match_resident([fr], [good])
        with pytest.raises(capi.OshError, match="frame 1: the token names no frame"):
            matcher.stereo_match_resident([fr, fr], [good, (good[0], 0)])                                    # the second frame of a call
    with orb.OrbMatcher(0) as fresh:                                                                       # no resident pyramid at all
        with pytest.raises(capi.OshError, match="names no frame"):
            fresh.stereo_match_resident([fr], [good])
    sn.assert_same(matcher.stereo_match_resident([fr], [good], stages=True)[0], st, what="after the refusals")
    # frames of different depth
    mixed = matcher.pyramid_build([items[0], dict(image=p["right"]["image"], inv_scale=sc.pair("pair_240x180_L4")["left"]["inv_scale"]), items[1]], download=False)
    with pytest.raises(capi.OshError, match="the left frame has 3 levels, the right frame 4, the call names 3"):
        matcher.stereo_match_resident([fr], [(mixed[0]["token"], mixed[1]["token"])])
    two = dataclasses.replace(fr, scale_factors=fr.scale_factors[:2], inv_scale_factors=fr.inv_scale_factors[:2], left_pyramid=fr.left_pyramid[:2],
                              right_pyramid=fr.right_pyramid[:2], left_octave=np.minimum(fr.left_octave, 1), right_octave=np.minimum(fr.right_octave, 1))
    with pytest.raises(capi.OshError, match="the left frame has 3 levels, the right frame 3, the call names 2"):
        matcher.stereo_match_resident([two], [(mixed[0]["token"], mixed[2]["token"])])
    sn.assert_same(matcher.stereo_match_resident([fr], [(mixed[0]["token"], mixed[2]["token"])], stages=True)[0], st, what="after the level refusals")


def test_the_tokens_of_the_fused_call_serve_the_later_stages(matcher):
    p = sc.pair("pair_240x180_L4")
    got = matcher.extract_stereo([p], stages=True)[0]
    for side in ("left", "right"):
        g = got[side]
        angle = matcher.ic_angle([dict(xy=g["xy"], level=g["level"], token=g["token"])])[0]["angle"]
        assert np.array_equal(angle.view(np.uint32), g["angle"].view(np.uint32)), side
        desc = matcher.describe([dict(xy=g["xy"], level=g["level"], angle=g["angle"], pattern=p[side]["pattern"], token=g["token"])])[0]["descriptors"]
        assert np.array_equal(desc, g["descriptors"]), side
    ex, fr, st = _expected("pair_240x180_L4")
    sn.assert_same(matcher.stereo_match_resident([fr], [(got["left"]["token"], got["right"]["token"])], stages=True)[0], st, what="the stage by the fused call's tokens")


def test_an_extract_after_the_fused_call_is_the_extract_it_was(matcher):
    """The tail lays the keypoints out left frames first; a call without a tail on the same context is back to frame after frame."""
    names = ("pair_240x180_L4", "pair_160x120_L3")
    items = [sc.pair(n)[side] for n in names for side in ("left", "right")]
    with orb.OrbMatcher(0) as untouched:
        exp = untouched.extract(items, download=True)
    matcher.extract_stereo([sc.pair(n) for n in names], stages=True)
    got = matcher.extract(items, download=True)
    for k, (g, e) in enumerate(zip(got, exp)):
        _same_extract(g, e, f"frame {k}")
        for l, (a, b) in enumerate(zip(g["bordered"], e["bordered"])):
            assert np.array_equal(a, b), f"frame {k} bordered level {l}"


def test_the_five_phase_times(matcher):
    p = sc.pair("pair_240x180_L4")
    matcher.set_profiling(True)
    try:
        matcher.extract_stereo([p])
        five, four = matcher.extract_stereo_times(), matcher.extract_times()
    finally:
        matcher.set_profiling(False)
    assert (five > 0).all() and five[4] < four[3]
    assert np.allclose(five[:3], four[:3]) and np.isclose(five[3] + five[4], four[3])


# ---------------------------------------------------------------------------------------------- 5. through the class
KEYPOINT_FIELDS = ("xy", "angle", "size", "response", "octave", "descriptors")


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    assert np.array_equal(a, b), f"{what} differs at {np.argwhere(a != b)[:5].tolist()}"


@pytest.mark.parametrize("raw", (False, True), ids=("grey", "raw"))
def test_the_member_equals_the_two_calls_it_replaces(hip_lib, raw):
    """Frame::ExtractAndMatchStereo against ExtractBatch(Raw) with bKeepPyramid and ComputeStereoMatches on a twin frame."""
    p = sp.named_pair("pair_240x180_L4")
    kw = dict(nfeatures=500, nlevels=4)
    colour = lambda im: dict(image=np.ascontiguousarray(np.repeat(im[:, :, None], 3, axis=2)), order="bgr")   # R = G = B: the grey value itself
    sides = (colour(p["left"]), colour(p["right"])) if raw else (p["left"], p["right"])
    got = host.frame_extract_and_match_stereo(*sides, p["bf"], p["b"], raw=raw, want_gray=raw, **kw)
    twin = host.frame_extract_and_match_stereo(*sides, p["bf"], p["b"], raw=raw, chain=True, want_gray=raw, **kw)
    for side in ("left", "right"):
        for k in KEYPOINT_FIELDS:
            _same_bits(got[side][k], twin[side][k], f"{side} {k}")
        assert got[side]["token"] != 0 and all(lv.size == 0 for lv in got[side]["pyramid"])         # as bKeepPyramid = false leaves them
        assert all(lv.size > 0 for lv in twin[side]["pyramid"])
        if raw:
            assert np.array_equal(got[side]["gray"], p[side]) and np.array_equal(twin[side]["gray"], p[side])
    assert got["left"]["token"] != got["right"]["token"]
    assert got["N"] == twin["N"] == len(got["left"]["octave"]) > 100 and got["n_right"] == len(got["right"]["octave"]) > 100
    _same_bits(got["u_right"], twin["u_right"], "mvuRight")
    _same_bits(got["depth"], twin["depth"], "mvDepth")
    assert len(got["depth"]) == got["N"] and (got["depth"] > 0).sum() * 4 >= got["N"]
    # and the keypoints are those of the fused call, scaled to level 0
    with orb.OrbMatcher(0) as m:
        fused = m.extract_stereo([sc.pair("pair_240x180_L4")])[0]
    _same_bits(got["left"]["xy"], sc.level0(fused["left"]["xy"], fused["left"]["level"], sc.scales(4)), "mvKeys against the fused call")
    _same_bits(got["u_right"], fused["stereo"]["u_right"], "mvuRight against the fused call")


def test_a_refused_call_leaves_the_frame_empty_after_a_message(hip_lib, capfd):
    p = sp.named_pair("pair_160x120_L3")
    kw = dict(nfeatures=300, nlevels=3)
    for what, args, needle in (("b = 0", (p["left"], p["right"], 40.0, 0.0), "bad bf / b"),
                               ("no right image", (p["left"], None, 40.0, 1.0), "two extractors with an image each")):
        capfd.readouterr()
        got = host.frame_extract_and_match_stereo(*args, **kw)
        err = capfd.readouterr().err
        assert "ExtractAndMatchStereo" in err and needle in err, (what, err)
        assert got["N"] == 0 and got["n_right"] == 0 and len(got["u_right"]) == 0 and len(got["depth"]) == 0, what
        assert len(got["left"]["octave"]) == 0 and len(got["right"]["octave"]) == 0 and got["left"]["desc_rows"] == 0, what
    good = host.frame_extract_and_match_stereo(p["left"], p["right"], 40.0, 1.0, **kw)            # the thread's context still serves
    assert good["N"] > 50 and len(good["u_right"]) == good["N"]


# ---------------------------------------------------------------------------------------------- 6. the row-list search
def test_row_lists_on_4000_and_4000_keypoints(matcher):
    fr = ss.make_stereo_frame(seed=9, n_left=4000, n_right=4000)
    assert len(fr.left_octave) == 4000 and len(fr.right_octave) == 4000
    got = _resident_against_brought(matcher, fr, "4000 + 4000")
    assert (got["stage"] == capi.OSH_STEREO_ACCEPTED).sum() > 400


def test_row_lists_with_every_right_keypoint_in_one_row(matcher):
    fr = ss.make_stereo_frame(seed=2)
    rxy = fr.right_xy.copy()
    rxy[:, 1] = F(211.25)
    lxy = fr.left_xy.copy()
    lxy[::3, 1] = F(212.5)                                                            # a third of the left keypoints look into that band
    one = dataclasses.replace(fr, right_xy=rxy, left_xy=lxy)
    got = _resident_against_brought(matcher, one, "one row")
    assert (got["stage"][::3] != capi.OSH_STEREO_NO_CANDIDATE).all() and (got["stage"] == capi.OSH_STEREO_NO_CANDIDATE).sum() > len(lxy) // 3


def test_both_searches_give_the_same_bits(matcher):
    """The switch of the search: the fused call and the resident stage with k_stereo_hamming equal themselves with the row lists."""
    p = sc.pair("pair_240x180_L4")
    ex, fr, st = _expected("pair_240x180_L4")
    try:
        for enable in (False, True):
            matcher.set_stereo_row_search(enable)
            got = matcher.extract_stereo([p], stages=True)[0]
            _same_pair(got, (ex, fr, st), f"row search {enable}")
            by_token = matcher.stereo_match_resident([fr], [(got["left"]["token"], got["right"]["token"])], stages=True)[0]
            sn.assert_same(by_token, st, what=f"resident, row search {enable}")
    finally:
        matcher.set_stereo_row_search(True)


def test_the_tail_behind_a_resize_of_colour_images(matcher):
    """The raw form with work for the front end: 3-channel images of another size, resized and turned grey before the extraction."""
    named = sp.named_pair("pair_240x180_L4")
    big = lambda im: np.ascontiguousarray(np.repeat(np.repeat(im, 2, axis=0), 2, axis=1)[:350, :470, None] * np.ones((1, 1, 3), np.uint8))
    base = sc.pair("pair_240x180_L4")
    p = dict(base, left=dict(base["left"], image=big(named["left"]), order="bgr", out_shape=(180, 240)),
             right=dict(base["right"], image=big(named["right"]), order="rgb", out_shape=(180, 240)))
    exp = _chain(matcher, p, raw=True)
    got = matcher.extract_stereo([p], stages=True, raw=True)[0]
    _same_pair(got, exp, "resized colour pair")
    assert got["left"]["n_out"] > 50 and got["right"]["n_out"] > 50
