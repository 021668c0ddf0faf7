"""osh_orb_extract and ORBextractor::ExtractBatch on the device against the chain of the existing calls on the same image:
osh_orb_pyramid_build, osh_orb_fast_detect_resident, the octree restatement of tests/octree_numpy.py, minBorder added,
osh_orb_ic_angle and osh_orb_describe by token.  Every output field bit for bit: the fused call runs the kernels of those calls."""
import functools

import numpy as np
import pytest

import octree_numpy as on
import pyramid_numpy as pn
from orb_slam3_study_kr_amd import capi, host, orb
from orb_slam3_study_kr_amd import synth_fast as sf

pytestmark = pytest.mark.gpu
F = np.float32


def _scales(nlevels, scale_factor=1.2):
    s = [F(1)]
    for _ in range(1, nlevels):
        s.append(F(s[-1] * F(scale_factor)))
    return np.asarray(s, F)


def _item(image, nlevels, nfeatures=1000, ini_th=20, min_th=7):
    return dict(image=np.ascontiguousarray(image, np.uint8), inv_scale=np.asarray(pn.standin_inv_scale(nlevels), F), scale=_scales(nlevels),
                n_features=np.asarray(on.features_per_level(nfeatures, 1.2, nlevels), np.int32), pattern=orb.standin_pattern(), ini_th=ini_th,
                min_th=min_th, border=19)


@functools.lru_cache(maxsize=None)
def _items():
    return dict(mix_160x120_L3=_item(sf.make_image(3, 120, 160), 3, nfeatures=300),
                low_th_240x180_L4=_item(sf.make_image(5, 180, 240), 4, nfeatures=500, ini_th=12, min_th=5),
                small_67x67_L4=_item(sf.make_image(17, 67, 67, density=3.0, flat_band=False, weak_band=False), 4, nfeatures=100),
                uniform_120x90_L3=_item(np.full((90, 120), 113, np.uint8), 3, nfeatures=200),
                vga_752x480_L8=_item(sf.make_image(31, 480, 752), 8, nfeatures=1000))


def _chain(m, it):
    """The existing calls one after another, the octree as the restatement; the keypoints never leave the host's hands."""
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
    n = int(level_count.sum())
    xy = np.concatenate(xy) if n else np.zeros((0, 2), F)
    level = np.concatenate(level) if n else np.zeros(0, np.int32)
    response = np.concatenate(response) if n else np.zeros(0, F)
    angle = m.ic_angle([dict(xy=xy, level=level, token=built["token"])])[0]["angle"] if n else np.zeros(0, F)
    desc = m.describe([dict(xy=xy, level=level, angle=angle, pattern=it["pattern"], token=built["token"])])[0]["descriptors"] if n else np.zeros((0, 32), np.uint8)
    size = np.asarray([F(int(F(31) * it["scale"][l])) for l in level], F)
    return dict(level_count=level_count, xy=xy, level=level, response=response, angle=angle, size=size, descriptors=desc, bordered=built["bordered"])


def _assert_same(got, exp, what, bordered=True):
    assert got["n_out"] == len(exp["level"]), f"{what}: {got['n_out']} keypoints, {len(exp['level'])} expected"
    for k in ("level_count", "xy", "level", "response", "angle", "size", "descriptors"):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, f"{what}: {k} shape {g.shape} != {e.shape}"
        if g.dtype == np.float32:
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(g, e), f"{what}: {k} differs at {np.argwhere(g != e)[:5].tolist()}"
    if bordered:
        for l, (g, e) in enumerate(zip(got["bordered"], exp["bordered"])):
            assert np.array_equal(g, e), f"{what}: bordered level {l}"


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


@functools.lru_cache(maxsize=None)
def _expected(name):
    with orb.OrbMatcher(0) as m:
        return _chain(m, _items()[name])


@pytest.mark.parametrize("name", ("mix_160x120_L3", "low_th_240x180_L4", "small_67x67_L4", "uniform_120x90_L3", "vga_752x480_L8"))
def test_the_fused_call_equals_the_chain(matcher, name):
    exp = _expected(name)
    got = matcher.extract([_items()[name]], download=True)[0]
    _assert_same(got, exp, name)
    if name == "uniform_120x90_L3":
        assert got["n_out"] == 0 and not got["level_count"].any()
    elif name == "small_67x67_L4":
        assert got["level_count"][0] > 0 and not got["level_count"][1:].any()      # the levels above have no cells
    else:
        assert (got["level_count"] > 0).all()
    if name == "vga_752x480_L8":
        assert 900 < got["n_out"] < 1100
    plain = matcher.extract([_items()[name]])[0]                                    # levels == NULL: nothing downloaded, same keypoints
    _assert_same(plain, exp, f"{name} without the levels", bordered=False)
    assert "bordered" not in plain


def test_a_batch_of_three_mixed_frames_equals_the_single_calls(matcher):
    names = ("low_th_240x180_L4", "uniform_120x90_L3", "mix_160x120_L3")
    batch = matcher.extract([_items()[n] for n in names], download=True)
    assert len({b["token"] for b in batch}) == 3
    for b, n in zip(batch, names):
        _assert_same(b, _expected(n), f"batch {n}")


def test_tokens_serve_a_later_ic_angle_and_describe(matcher):
    it = _items()["mix_160x120_L3"]
    got = matcher.extract([it, _items()["low_th_240x180_L4"]])
    for g, name in zip(got, ("mix_160x120_L3", "low_th_240x180_L4")):
        ang = matcher.ic_angle([dict(xy=g["xy"], level=g["level"], token=g["token"])])[0]["angle"]
        assert np.array_equal(ang.view(np.uint32), g["angle"].view(np.uint32)), name
        desc = matcher.describe([dict(xy=g["xy"], level=g["level"], angle=g["angle"], pattern=it["pattern"], token=g["token"])])[0]["descriptors"]
        assert np.array_equal(desc, g["descriptors"]), name


def test_overflow_convention_and_refusals(matcher):
    it = _items()["mix_160x120_L3"]
    exp = _expected("mix_160x120_L3")
    n = len(exp["level"])
    got = matcher.extract([it, it], capacities=[n - 1, n])
    assert got[0]["n_out"] == n and got[0]["xy"] is None and np.array_equal(got[0]["level_count"], exp["level_count"])
    _assert_same(got[1], exp, "exact capacity", bordered=False)
    token = got[1]["token"]
    far = it["pattern"].copy()
    far[0] = (15, 15)                                                               # reaches 22 pixels: beyond a kept corner's margin
    for what, bad, code in (("threshold", dict(it, ini_th=0), capi.OSH_ERR_INVALID), ("min above ini", dict(it, ini_th=5, min_th=9), capi.OSH_ERR_INVALID),
                            ("features above the limit", dict(it, n_features=np.asarray([5000, 10, 10], np.int32)), capi.OSH_ERR_UNSUPPORTED),
                            ("table reach", dict(it, pattern=far), capi.OSH_ERR_INVALID),
                            ("blur weights", dict(it, blur_q8=np.asarray([1, 2, 3, 4, 3, 2, 1], np.uint16)), capi.OSH_ERR_INVALID),
                            ("inv_scale", dict(it, inv_scale=np.asarray([1, -1, 0.5], F)), capi.OSH_ERR_INVALID)):
        with pytest.raises(capi.OshError) as err:
            matcher.extract([it, bad], capacities=[n, n])
        assert err.value.code == code, what
    # a refused call leaves the resident pyramid as it was: the old token still serves
    ang = matcher.ic_angle([dict(xy=exp["xy"], level=exp["level"], token=token)])[0]["angle"]
    assert np.array_equal(ang.view(np.uint32), exp["angle"].view(np.uint32))


def _write_back(g, scale, lapping):
    """:1143-1164 in numpy: scale to level 0, keypoints of the lapping area from the back, the others from the front."""
    n = g["n_out"]
    xy, order, mono, stereo = g["xy"].copy(), np.zeros(n, np.int64), 0, n - 1
    for i in range(n):
        if g["level"][i] != 0:
            xy[i] = xy[i] * scale[g["level"][i]]
        if lapping[0] <= xy[i, 0] <= lapping[1]:
            order[stereo] = i; stereo -= 1
        else:
            order[mono] = i; mono += 1
    return xy[order], order, mono


@pytest.mark.parametrize("keep", (True, False))
def test_extract_batch_of_a_left_and_right_pair(matcher, keep):
    left, right = sf.make_image(3, 120, 160), sf.make_image(4, 120, 160)
    lappings = [(0, 60), (100, 159)]
    items = [_item(im, 3, nfeatures=300) for im in (left, right)]
    fused = matcher.extract(items, download=True)
    got = host.orbextractor_extract_batch([left, right, None], lappings + [(0, 0)], nfeatures=300, nlevels=3, keep_pyramid=keep)
    assert got[2]["ret"] == -1 and got[2]["desc_rows"] == 2 and got[2]["token"] == 0          # an empty image: nothing touched, as operator()
    assert got[0]["token"] and got[1]["token"] == got[0]["token"] + 1                         # one call, consecutive frames
    for k in range(2):
        g, f = got[k], fused[k]
        xy, order, mono = _write_back(f, items[k]["scale"], lappings[k])
        assert g["ret"] == mono and 0 < mono < f["n_out"] and g["desc_rows"] == f["n_out"]
        assert np.array_equal(g["xy"].view(np.uint32), xy.view(np.uint32))
        for name in ("angle", "size", "response"):
            assert np.array_equal(g[name].view(np.uint32), f[name][order].view(np.uint32)), name
        assert np.array_equal(g["octave"], f["level"][order]) and np.array_equal(g["descriptors"], f["descriptors"][order])
        if keep:
            for a, b in zip(g["pyramid"], f["levels"]):
                assert np.array_equal(a, b)
        else:
            assert all(p.size == 0 for p in g["pyramid"])


@pytest.mark.parametrize("keep", (True, False))
def test_extract_batch_refuses_an_image_whose_level_rounds_to_no_pixels(matcher, capfd, keep):
    # 40 rows by 1 column, 8 levels at 1.2: the width of level 4 is nearbyint(1 * 0.48225) = 0.  The valid frame beside it gets
    # nothing either: one refused extractor refuses the call
    tall, valid = np.full((40, 1), 90, np.uint8), sf.make_image(3, 120, 160)
    capfd.readouterr()
    got = host.orbextractor_extract_batch([tall, valid], [(0, 0), (0, 60)], nfeatures=300, nlevels=8, keep_pyramid=keep)
    err = capfd.readouterr().err
    if keep:   # ExtractBatch sizes the levels it keeps and refuses by itself
        assert "ORBextractor::ExtractBatch: extractor 0: level 4 has no pixels or too many" in err
        assert "ORBextractor::ExtractBatch: nothing extracted" in err
    else:      # the pyramid stage of osh_orb_extract refuses
        assert "ORBextractor::ExtractBatch: osh_orb_pyramid_build: frame 0: level 4 rounds to 0 pixels in a direction" in err
        assert "nothing extracted" not in err
    for g in got:
        assert g["ret"] == 0 and g["desc_rows"] == 0 and g["token"] == 0
        assert len(g["xy"]) == 0 and len(g["descriptors"]) == 0
        assert len(g["pyramid"]) == 8 and all(p.size == 0 for p in g["pyramid"])


def test_phase_times(matcher):
    matcher.set_profiling(True)
    try:
        matcher.extract([_items()["mix_160x120_L3"]])
        ms = matcher.extract_times()
    finally:
        matcher.set_profiling(False)
    assert ms.shape == (4,) and (ms > 0).all()
