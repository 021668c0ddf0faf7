"""The image front end on the device: osh_orb_prepare against the numpy restatement of tests/prepare_numpy.py bit for bit,
osh_orb_extract_raw against osh_orb_extract fed with the image osh_orb_prepare downloaded, ORBextractor::ExtractBatchRaw against
ExtractBatch on the prepared images, rectify maps shared between contexts, and the entries around them after the split of the
pyramid body.  No test provokes a device fault: the edge cases are inputs the definition covers."""
import ctypes as C

import numpy as np
import pytest

import octree_numpy as on
import prepare_numpy as pp
import pyramid_numpy as pn
from orb_slam3_study_kr_amd import capi, host, orb
from orb_slam3_study_kr_amd import synth_fast as sf

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


@pytest.fixture(scope="module")
def maps(matcher):
    """One resident map per committed case that has one, and per extra key a test adds; closed at the end."""
    made = {}

    def get(key, map_x=None, map_y=None, src_shape=None):
        if key not in made:
            if map_x is None:
                it = pp.item(key)
                map_x, map_y, src_shape = it["map_x"], it["map_y"], it["image"].shape[:2]
            made[key] = matcher.rectify_map(map_x, map_y, src_shape)
        return made[key]
    yield get
    for m in made.values():
        m.close()


def _orb_item(name, maps, image=None):
    it = pp.item(name)
    return dict(image=it["image"] if image is None else image, order=it["order"], map=None if it["map_x"] is None else maps(name),
                out_shape=it["out_shape"])


def _strided(img):
    whole = np.full((img.shape[0] + 3, img.shape[1] + 6) + img.shape[2:], 91, img.dtype)
    view = whole[2:2 + img.shape[0], 5:5 + img.shape[1]]
    view[...] = img
    return view


@pytest.mark.parametrize("name", pp.CASE_NAMES)
def test_prepare_equals_the_restatement(matcher, maps, name):
    exp = pp.expected(name)
    got = matcher.prepare([_orb_item(name, maps)])[0]
    assert got["shape"] == exp.shape
    pp.assert_same(got["gray"], exp, name)
    assert (got["gray_whole"][:, exp.shape[1]:] == 167).all(), "written beyond the row"
    got = matcher.prepare([_orb_item(name, maps, image=_strided(pp.item(name)["image"]))])[0]
    pp.assert_same(got["gray"], exp, name + " strided")
    got = matcher.prepare([_orb_item(name, maps)], download=False)[0]          # nothing downloaded: the size alone
    assert got["shape"] == exp.shape and "gray" not in got


def test_prepare_on_a_large_frame(matcher, maps):
    got = matcher.prepare([_orb_item(pp.LARGE, maps)])[0]
    pp.assert_same(got["gray"], pp.expected(pp.LARGE), pp.LARGE)


def test_a_batch_of_five_mixed_frames_equals_the_single_calls(matcher, maps):
    names = ("rgb_remap_37x53", "passthrough_1x50", "resize_37x53_to_30x41_c3", "gray_bgra_5x7", "remap_17x65_from_23x70")
    got = matcher.prepare([_orb_item(n, maps) for n in names])
    for n, g in zip(names, got):
        pp.assert_same(g["gray"], pp.expected(n), f"batch {n}")
    # some want their image, some do not
    cf, cr, _m, _keep, outs = orb.prepare_args([_orb_item(n, maps) for n in names], True)
    for k in (1, 3):
        cr[k].gray = C.cast(None, capi.c_uint8_p)
    capi.check(matcher.lib.osh_orb_prepare(matcher.ctx, len(names), cf, cr), "osh_orb_prepare", matcher.lib)
    for k, n in enumerate(names):
        assert (int(cr[k].rows), int(cr[k].cols)) == pp.expected(n).shape
        if k in (1, 3):
            assert (outs[k]["gray_whole"] == 167).all()
        else:
            pp.assert_same(outs[k]["gray"], pp.expected(n), f"partial download {n}")


def test_one_map_serves_two_contexts_and_a_recreated_map_gives_the_same_bits(matcher, maps):
    name = "rgb_remap_37x53"
    exp = pp.expected(name)
    with orb.OrbMatcher(0) as other:
        a = matcher.prepare([_orb_item(name, maps)])[0]["gray"]
        b = other.prepare([_orb_item(name, maps)])[0]["gray"]
        c = matcher.prepare([_orb_item(name, maps)])[0]["gray"]
    for g in (a, b, c):
        pp.assert_same(g, exp, name)
    it = pp.item(name)
    for _ in range(2):
        with matcher.rectify_map(it["map_x"], it["map_y"], it["image"].shape[:2]) as m:
            got = matcher.prepare([dict(image=it["image"], order=it["order"], map=m)])[0]["gray"]
        pp.assert_same(got, exp, name + " re-created")


def test_refusals_that_need_a_map(matcher, maps):
    it = pp.item("rgb_remap_37x53")                                  # a 37 x 53 map for a 41 x 57 source
    m = maps("rgb_remap_37x53")
    before = matcher.pyramid_build([pn.item("chain_37x53")])[0]
    for bad, needle in ((dict(image=it["image"][:40], map=m), "the map was made for a 41 x 57 source, the image is 40 x 57"),
                        (dict(image=it["image"], map=m, out_shape=(37, 52)), "the output size 37 x 52 is not the map's 37 x 53"),
                        (dict(image=it["image"], map=m, out_shape=(0, 53)), "is not positive")):
        with pytest.raises(capi.OshError) as err:
            matcher.prepare([bad])
        assert err.value.code == capi.OSH_ERR_INVALID and needle in str(err.value), str(err.value)
        cf, cr, *_ = orb.prepare_args([bad], True)
        assert matcher.lib.osh_orb_prepare(None, 1, cf, cr) == capi.OSH_ERR_INVALID and needle in capi.last_error(matcher.lib)   # without a context
    # the refused calls left the resident pyramid alone
    exp = pn.case("chain_37x53")[1]
    lv = exp["levels"][1]
    xy, level = np.asarray([[lv.shape[1] // 2, lv.shape[0] // 2]], F), np.asarray([1], np.int32)
    a = matcher.ic_angle([dict(xy=xy, level=level, token=before["token"])])[0]["angle"]
    b = matcher.ic_angle([dict(xy=xy, level=level, pyramid=exp["levels"])])[0]["angle"]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- osh_orb_extract_raw

def _scales(nlevels, scale_factor=1.2):
    s = [F(1)]
    for _ in range(1, nlevels):
        s.append(F(s[-1] * F(scale_factor)))
    return np.asarray(s, F)


def _extract_keys(nlevels, nfeatures):
    return dict(inv_scale=np.asarray(pn.standin_inv_scale(nlevels), F), scale=_scales(nlevels),
                n_features=np.asarray(on.features_per_level(nfeatures, 1.2, nlevels), np.int32), pattern=orb.standin_pattern(), ini_th=20, min_th=7,
                border=19)


def _colour(seed, rows, cols):
    """Three channels with corners of their own each."""
    return np.ascontiguousarray(np.stack([sf.make_image(seed + k, rows, cols) for k in range(3)], -1))


def _raw_items(maps):
    """name -> the items of one extract_raw call."""
    mx, my = pp.rectify_maps(120, 160, (130, 170))
    rgb = dict(image=_colour(40, 130, 170), order="rgb", map=maps("rgb_120x160", mx, my, (130, 170)), **_extract_keys(3, 300))
    lx, ly = pp.rectify_maps(120, 160, (120, 160), tilt=0.02)
    rx, ry = pp.rectify_maps(120, 160, (124, 166), tilt=-0.015, k1=-0.2, shift=(2.5, 1.25))
    left = dict(image=np.ascontiguousarray(sf.make_image(3, 120, 160)), map=maps("left_120x160", lx, ly, (120, 160)), **_extract_keys(3, 300))
    right = dict(image=_colour(50, 124, 166), order="bgr", map=maps("right_120x160", rx, ry, (124, 166)), **_extract_keys(4, 250))
    big = pp.item(pp.LARGE)
    euroc = dict(image=big["image"], map=maps(pp.LARGE), **_extract_keys(8, 1000))
    return dict(rgb_remap_120x160=[rgb], stereo_pair=[left, right], euroc_752x480=[euroc])


def _same_extraction(got, exp, what, bordered=True):
    assert got["n_out"] == exp["n_out"], f"{what}: {got['n_out']} keypoints, {exp['n_out']} expected"
    for k in ("level_count", "xy", "level", "response", "angle", "size", "descriptors"):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, f"{what}: {k} shape {g.shape} != {e.shape}"
        if g.dtype == np.float32:
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(g, e), f"{what}: {k} differs at {np.argwhere(g != e)[:5].tolist()}"
    if bordered:
        assert len(got["bordered"]) == len(exp["bordered"])
        for l, (g, e) in enumerate(zip(got["bordered"], exp["bordered"])):
            assert np.array_equal(g, e), f"{what}: bordered level {l}"


@pytest.mark.parametrize("name", ("rgb_remap_120x160", "stereo_pair", "euroc_752x480"))
def test_extract_raw_equals_extract_on_the_prepared_image(matcher, maps, name):
    items = _raw_items(maps)[name]
    prepared = [np.ascontiguousarray(p["gray"]) for p in matcher.prepare(items)]
    exp = matcher.extract([dict(it, image=g) for it, g in zip(items, prepared)], download=True)
    got = matcher.extract_raw(items, download=True, gray=True)
    assert len({g["token"] for g in got}) == len(items) and all(g["token"] for g in got)
    for k, (g, e) in enumerate(zip(got, exp)):
        _same_extraction(g, e, f"{name} frame {k}")
        assert g["n_out"] > 20 and (g["level_count"] > 0).all(), (name, g["level_count"])      # not an empty comparison
        assert g["shape"] == prepared[k].shape
        pp.assert_same(g["gray"], prepared[k], f"{name} frame {k} gray")
        assert np.array_equal(g["levels"][0], prepared[k])
    plain = matcher.extract_raw(items)                                              # nothing but the keypoints comes back
    for k, (g, e) in enumerate(zip(plain, exp)):
        _same_extraction(g, e, f"{name} frame {k} without the levels", bordered=False)
        assert "bordered" not in g and "gray" not in g
    # the tokens serve a later osh_orb_ic_angle / osh_orb_describe
    for g, it in zip(plain, items):
        ang = matcher.ic_angle([dict(xy=g["xy"], level=g["level"], token=g["token"])])[0]["angle"]
        assert np.array_equal(ang.view(np.uint32), g["angle"].view(np.uint32))
        desc = matcher.describe([dict(xy=g["xy"], level=g["level"], angle=g["angle"], pattern=it["pattern"], token=g["token"])])[0]["descriptors"]
        assert np.array_equal(desc, g["descriptors"])


def _chain(m, it):
    """osh_orb_extract restated as the chain of the stage calls, the octree as tests/octree_numpy.py restates it."""
    built = m.pyramid_build([it])[0]
    nl = len(it["inv_scale"])
    det = m.fast_detect_resident([dict(token=built["token"], n_levels=nl, ini_th=it["ini_th"], min_th=it["min_th"])])[0]
    xy, level, response, level_count = [], [], [], np.zeros(nl, np.int32)
    for l, (rows, cols) in enumerate(built["shapes"]):
        sel = det["level"] == l
        if not sel.any():
            continue
        cxy, cr = det["xy"][sel], det["response"][sel]
        kept = on.distribute(cxy, cr, cols - 32, rows - 32, int(it["n_features"][l]))[0]
        xy.append(cxy[kept] + F(16)); response.append(cr[kept]); level.append(np.full(len(kept), l, np.int32))
        level_count[l] = len(kept)
    xy, level, response = np.concatenate(xy), np.concatenate(level), np.concatenate(response)
    angle = m.ic_angle([dict(xy=xy, level=level, token=built["token"])])[0]["angle"]
    desc = m.describe([dict(xy=xy, level=level, angle=angle, pattern=it["pattern"], token=built["token"])])[0]["descriptors"]
    size = np.asarray([F(int(F(31) * it["scale"][l])) for l in level], F)
    return dict(n_out=len(level), level_count=level_count, xy=xy, level=level, response=response, angle=angle, size=size, descriptors=desc,
                bordered=built["bordered"])


def test_extract_and_pyramid_build_after_an_extract_raw_equal_their_restatements(matcher, maps):
    matcher.extract_raw(_raw_items(maps)["stereo_pair"])
    it, exp = pn.case("chain_37x53")
    pn.assert_same(matcher.pyramid_build([it])[0], exp, "pyramid_build after extract_raw")
    matcher.extract_raw(_raw_items(maps)["rgb_remap_120x160"])
    it, exp = pn.case("halving_40x64")
    pn.assert_same(matcher.pyramid_build([it, pn.item("tile_17x65")])[0], exp, "pyramid_build of two frames after extract_raw")
    matcher.extract_raw(_raw_items(maps)["stereo_pair"])
    plain = dict(image=np.ascontiguousarray(sf.make_image(3, 120, 160)), **_extract_keys(3, 300))
    got = matcher.extract([plain], download=True)[0]
    _same_extraction(got, _chain(matcher, plain), "extract after extract_raw")
    assert np.array_equal(got["levels"][0], plain["image"])


def test_a_refused_extract_raw_leaves_the_earlier_token_valid(matcher, maps):
    items = _raw_items(maps)["rgb_remap_120x160"]
    good = matcher.extract_raw(items)[0]
    n = good["n_out"]
    far = items[0]["pattern"].copy()
    far[0] = (15, 15)
    for what, bad, code in (("the output size", dict(items[0], out_shape=(100, 100)), capi.OSH_ERR_INVALID),
                            ("channel order", dict(items[0], order=7), capi.OSH_ERR_INVALID),
                            ("threshold", dict(items[0], ini_th=0), capi.OSH_ERR_INVALID),
                            ("features above the limit", dict(items[0], n_features=np.asarray([5000, 10, 10], np.int32)), capi.OSH_ERR_UNSUPPORTED),
                            ("table reach", dict(items[0], pattern=far), capi.OSH_ERR_INVALID),
                            ("inv_scale", dict(items[0], inv_scale=np.asarray([1, -1, 0.5], F)), capi.OSH_ERR_INVALID)):
        with pytest.raises(capi.OshError) as err:
            matcher.extract_raw([items[0], bad], capacities=[n, n])
        assert err.value.code == code, what
    ang = matcher.ic_angle([dict(xy=good["xy"], level=good["level"], token=good["token"])])[0]["angle"]
    assert np.array_equal(ang.view(np.uint32), good["angle"].view(np.uint32))
    # the overflow convention is osh_orb_extract's
    got = matcher.extract_raw([items[0], items[0]], capacities=[n - 1, n])
    assert got[0]["n_out"] == n and got[0]["xy"] is None and np.array_equal(got[0]["level_count"], good["level_count"])
    _same_extraction(got[1], good, "exact capacity", bordered=False)


# ---- ORBextractor::ExtractBatchRaw

def _pair():
    lx, ly = pp.rectify_maps(120, 160, (120, 160), tilt=0.02)
    rx, ry = pp.rectify_maps(120, 160, (124, 166), tilt=-0.015, k1=-0.2, shift=(2.5, 1.25))
    return [dict(image=_colour(60, 120, 160), order="bgr", map_x=lx, map_y=ly), dict(image=np.ascontiguousarray(sf.make_image(4, 124, 166)), map_x=rx, map_y=ry)]


@pytest.mark.parametrize("keep", (True, False))
def test_extract_batch_raw_of_a_left_and_right_pair(matcher, keep):
    pair = _pair()
    lappings = [(0, 60), (100, 159)]
    prepared = []
    for it in pair:
        with matcher.rectify_map(it["map_x"], it["map_y"], it["image"].shape[:2]) as m:
            prepared.append(np.ascontiguousarray(matcher.prepare([dict(image=it["image"], order=it.get("order", "rgb"), map=m)])[0]["gray"]))
    exp = host.orbextractor_extract_batch(prepared + [None], lappings + [(0, 0)], nfeatures=300, nlevels=3, keep_pyramid=keep)
    got = host.orbextractor_extract_batch_raw(pair + [dict(image=None)], lappings + [(0, 0)], nfeatures=300, nlevels=3, keep_pyramid=keep)
    assert got[2]["ret"] == -1 and got[2]["desc_rows"] == 2 and got[2]["token"] == 0 and got[2]["gray"] is None   # an empty image: nothing touched
    assert got[0]["token"] and got[1]["token"] == got[0]["token"] + 1
    for k in range(2):
        g, e = got[k], exp[k]
        # more than 20 keypoints, some on either side of the lapping bound (as the operator() tests ask of a 120 x 160 image): the
        # comparison is not an empty one
        assert g["ret"] == e["ret"] and g["desc_rows"] == e["desc_rows"] > 20 and 0 < g["ret"] < g["desc_rows"]
        for name in ("xy", "angle", "size", "response"):
            assert np.array_equal(g[name].view(np.uint32), e[name].view(np.uint32)), name
        assert np.array_equal(g["octave"], e["octave"]) and np.array_equal(g["descriptors"], e["descriptors"])
        assert len(g["pyramid"]) == len(e["pyramid"]) == 3
        for a, b in zip(g["pyramid"], e["pyramid"]):
            assert np.array_equal(a, b)
        if keep:
            assert np.array_equal(g["pyramid"][0], prepared[k])
        else:
            assert all(p.size == 0 for p in g["pyramid"])
        assert np.array_equal(g["gray"], prepared[k])
    without = host.orbextractor_extract_batch_raw(pair, lappings, nfeatures=300, nlevels=3, keep_pyramid=keep, want_gray=False)
    for g, e in zip(without, exp):
        assert g["ret"] == e["ret"] and np.array_equal(g["descriptors"], e["descriptors"])


@pytest.mark.parametrize("keep", (True, False))
def test_a_refused_extract_batch_raw_leaves_no_keypoints_and_says_why(matcher, capfd, keep):
    pair = _pair()
    pair[1] = dict(pair[1], out_shape=(100, 100))                 # a map and another output size
    capfd.readouterr()
    got = host.orbextractor_extract_batch_raw(pair, [(0, 60), (100, 159)], nfeatures=300, nlevels=3, keep_pyramid=keep)
    err = capfd.readouterr().err
    assert "ORBextractor::ExtractBatchRaw: osh_orb_extract_raw: frame 1: the output size 100 x 100 is not the map's 120 x 160" in err
    for g in got:
        assert g["ret"] == 0 and g["desc_rows"] == 0 and g["token"] == 0 and g["gray"] is None
        assert len(g["xy"]) == 0 and len(g["descriptors"]) == 0 and all(p.size == 0 for p in g["pyramid"])


def test_phase_times(matcher, maps):
    matcher.set_profiling(True)
    try:
        matcher.prepare([_orb_item("rgb_remap_37x53", maps)])
        ms = matcher.prepare_times()
        matcher.extract_raw(_raw_items(maps)["rgb_remap_120x160"])
        ems = matcher.extract_times()
    finally:
        matcher.set_profiling(False)
    assert ms.shape == (4,) and (ms >= 0).all() and ms[2] > 0
    assert ems.shape == (4,) and (ems >= 0).all() and ems[0] > 0
