"""The image front end without a GPU: the host build of csrc/orb_prepare.h (the statements k_prepare runs, osh_host_orb_prepare_cpu)
against the numpy restatement of tests/prepare_numpy.py bit for bit, what the definition fixes about the committed cases, the refusals
of osh_orb_prepare, osh_orb_extract_raw and osh_rectify_map_create that need no device, the export lists and the sanitizer program.
The refusals that need a rectify map object (a source size that is not the image's, an output size that is not the map's) need a
device to make one: tests/test_gpu_prepare.py holds them."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import prepare_numpy as pp
import pyramid_numpy as pn
from orb_slam3_study_kr_amd import capi, orb

F = np.float32
CSRC = capi.LIB_PATH.parent


def orb_item(it, device=None, **kw):
    """The item of orb.prepare / orb.prepare_cpu for an item of prepare_numpy; device None: the map is a description only."""
    m = None if it["map_x"] is None else orb.RectifyMap(it["map_x"], it["map_y"], it["image"].shape[:2], device)
    return dict(image=it["image"], order=it["order"], map=m, out_shape=it["out_shape"], **kw)


def strided(img):
    """The same pixels as a view into a larger array, rows further apart."""
    whole = np.full((img.shape[0] + 3, img.shape[1] + 6) + img.shape[2:], 91, img.dtype)
    view = whole[2:2 + img.shape[0], 5:5 + img.shape[1]]
    view[...] = img
    return view


def test_the_restatement_gives_the_known_answers():
    pp.check_known_answers()


@pytest.mark.parametrize("name", pp.CASE_NAMES)
def test_host_build_equals_the_restatement(name):
    it, exp = pp.case(name)
    got, _ = orb.prepare_cpu([orb_item(it)])
    assert got[0]["shape"] == exp.shape
    pp.assert_same(got[0]["gray"], exp, name)
    assert (got[0]["gray_whole"][:, exp.shape[1]:] == 167).all(), "written beyond the row"
    # the image and the maps as views with rows further apart
    it2 = dict(it, image=strided(it["image"]))
    if it["map_x"] is not None:
        it2.update(map_x=strided(it["map_x"]), map_y=strided(it["map_y"]))
    got, _ = orb.prepare_cpu([orb_item(it2)])
    pp.assert_same(got[0]["gray"], exp, name + " strided")


def test_host_build_on_a_large_frame():
    it, exp = pp.case(pp.LARGE)
    got, ms = orb.prepare_cpu([orb_item(it)])
    print(f"host build, 752x480 grey + remap on one thread: {ms:.2f} ms")
    pp.assert_same(got[0]["gray"], exp, pp.LARGE)


def test_host_build_of_a_batch_equals_the_single_calls():
    names = ("rgb_remap_37x53", "passthrough_1x50", "resize_37x53_to_30x41_c3", "gray_bgra_5x7", "remap_edges_12x20")
    got, _ = orb.prepare_cpu([orb_item(pp.item(n)) for n in names])
    for n, g in zip(names, got):
        pp.assert_same(g["gray"], pp.expected(n), n)


def _args(it, **kw):
    return orb.prepare_args([dict(orb_item(it), **kw)], True)


def test_prepare_refusals_need_no_device():
    lib = capi.load_library()
    host = capi.load_host_library()
    base = pp.item("gray_rgb_5x7")

    def refused(cf, cr, needle, code=capi.OSH_ERR_INVALID):
        rc = lib.osh_orb_prepare(None, 1, cf, cr)
        assert rc == code, (rc, needle, capi.last_error(lib))
        assert needle in capi.last_error(lib), (needle, capi.last_error(lib))
        assert host.osh_host_orb_prepare_cpu(1, cf, None, cr, None) == code, needle      # the host build refuses the same
        # the fused call refuses the same before it looks at anything else
        ef = (capi.ExtractFrame * 1)()
        er = (capi.ExtractResult * 1)()
        assert lib.osh_orb_extract_raw(None, 1, cf, ef, er, cr) == code and needle in capi.last_error(lib), capi.last_error(lib)

    cf, cr, *_ = _args(base)
    cf[0].image.data = C.cast(None, capi.c_uint8_p)
    refused(cf, cr, "the image is NULL or empty")
    for field in ("rows", "cols"):
        for v in (0, -3):
            cf, cr, *_ = _args(base)
            setattr(cf[0].image, field, v)
            refused(cf, cr, "the image is NULL or empty")
    cf, cr, *_ = _args(base)
    cf[0].image.stride = 7 * 3 - 1
    refused(cf, cr, "stride < cols * channels")
    for ch in (0, 2, 5, -1):
        cf, cr, *_ = _args(base)
        cf[0].image.channels = ch
        refused(cf, cr, f"{ch} channels, not 1, 3 or 4")
    for order in (2, -1):
        cf, cr, *_ = _args(base)
        cf[0].order = order
        refused(cf, cr, f"unknown channel order {order}")
    for shape in ((0, 7), (5, 0), (-1, -1), (-5, 7)):
        cf, cr, *_ = _args(base)
        cf[0].out_rows, cf[0].out_cols = shape
        refused(cf, cr, "is not positive")
    cf, cr, *_ = _args(base)
    cr[0].gray_stride = 6
    refused(cf, cr, "gray stride < cols")
    cf, cr, *_ = _args(base, out_shape=(9, 12))
    cr[0].gray_stride = 11
    refused(cf, cr, "gray stride < cols")
    cf, cr, *_ = _args(base)
    cf[0].image.rows = capi.OSH_FAST_MAX_SIDE + 1      # never read: refused first
    refused(cf, cr, "exceeds", capi.OSH_ERR_UNSUPPORTED)
    cf, cr, *_ = _args(base)
    cf[0].out_rows, cf[0].out_cols = 5, capi.OSH_FAST_MAX_SIDE + 1
    cr[0].gray_stride = capi.OSH_FAST_MAX_SIDE + 1
    refused(cf, cr, "exceeds", capi.OSH_ERR_UNSUPPORTED)
    assert lib.osh_orb_prepare(None, 1, None, None) == capi.OSH_ERR_INVALID and "bad arguments" in capi.last_error(lib)
    assert lib.osh_orb_prepare(None, -1, None, None) == capi.OSH_ERR_INVALID
    # what passes gets as far as the missing context
    for name in ("gray_rgb_5x7", "gray_bgra_5x7", "passthrough_1x50", "resize_37x53_to_30x41_c3", "resize_40x64_to_20x32_c1"):
        cf, cr, *_ = _args(pp.item(name))
        assert lib.osh_orb_prepare(None, 1, cf, cr) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib), name
    assert lib.osh_orb_prepare_get_times(None, None) == capi.OSH_ERR_INVALID


def _extract_item(it, nlevels=2):
    return dict(it, inv_scale=np.asarray(pn.standin_inv_scale(nlevels), F), scale=np.asarray([1 / s for s in pn.standin_inv_scale(nlevels)], F),
                n_features=np.full(nlevels, 50, np.int32), pattern=orb.standin_pattern())


def test_extract_raw_refusals_need_no_device():
    lib = capi.load_library()
    it = _extract_item(orb_item(pp.item("resize_37x53_to_30x41_c3")))

    def call(change=None, needle="no context", code=capi.OSH_ERR_INVALID):
        pf, pr, *_ = orb.prepare_args([it], True)
        cf, cr, _keep, _ = orb.extract_raw_args([it], [0])
        if change:
            change(pf, cf, cr)
        rc = lib.osh_orb_extract_raw(None, 1, pf, cf, cr, pr)
        assert rc == code and needle in capi.last_error(lib), (rc, needle, capi.last_error(lib))

    call()                                                       # what passes gets as far as the missing context
    pixels = np.zeros((30, 41), np.uint8)

    def brings_data(pf, cf, cr):
        cf[0].image.data = C.cast(pixels.ctypes.data, capi.c_uint8_p)
    call(brings_data, "brings image data")

    def other_size(pf, cf, cr):
        cf[0].image.rows, cf[0].image.cols = 37, 53              # the raw size is not the prepared size
    call(other_size, "names a 37 x 53 image, the prepared image is 30 x 41")

    def no_size(pf, cf, cr):
        cf[0].image.rows = cf[0].image.cols = 0                  # 0, 0: the prepared size
    call(no_size)

    def half_size(pf, cf, cr):
        cf[0].image.rows = 0
    call(half_size, "names a 0 x 41 image")

    # osh_orb_extract's own refusals, word for word
    def threshold(pf, cf, cr):
        cf[0].ini_th = 0
    call(threshold, "threshold outside [1, 255]")

    def levels(pf, cf, cr):
        cf[0].n_levels = 17
    call(levels, "n_levels 17 outside [1, 16]")

    def features(pf, cf, cr):
        it["n_features"][1] = capi.OSH_OCTREE_MAX_FEATURES + 1
    try:
        call(features, "above OSH_OCTREE_MAX_FEATURES", capi.OSH_ERR_UNSUPPORTED)
    finally:
        it["n_features"][1] = 50
    assert lib.osh_orb_extract_raw(None, 1, None, None, None, None) == capi.OSH_ERR_INVALID and "bad arguments" in capi.last_error(lib)


def test_rectify_map_create_refusals_and_no_device():
    lib = capi.load_library()
    mx, my = pp.rectify_maps(6, 9, (8, 11))
    m = orb.RectifyMap(mx, my, (8, 11))

    def rc(change=None, out=True):
        d = m.desc()
        if change:
            change(d)
        h = C.c_void_p()
        code = lib.osh_rectify_map_create(0, C.byref(d), C.byref(h) if out else None)
        assert not h
        return code

    assert rc(out=False) == capi.OSH_ERR_INVALID and "out is NULL" in capi.last_error(lib)
    h = C.c_void_p()
    assert lib.osh_rectify_map_create(0, None, C.byref(h)) == capi.OSH_ERR_INVALID and "NULL descriptor or map" in capi.last_error(lib)
    for field in ("map_x", "map_y"):
        assert rc(lambda d: setattr(d, field, C.cast(None, capi.c_float_p))) == capi.OSH_ERR_INVALID and "NULL descriptor or map" in capi.last_error(lib)
    for field in ("rows", "cols", "src_rows", "src_cols"):
        for v in (0, -2):
            assert rc(lambda d: setattr(d, field, v)) == capi.OSH_ERR_INVALID and "not positive" in capi.last_error(lib), field
        assert rc(lambda d: (setattr(d, field, capi.OSH_FAST_MAX_SIDE + 1), setattr(d, "map_x_stride", 1 << 20), setattr(d, "map_y_stride", 1 << 20))) \
            == capi.OSH_ERR_UNSUPPORTED and "exceeds" in capi.last_error(lib), field
    for field in ("map_x_stride", "map_y_stride"):
        assert rc(lambda d: setattr(d, field, 4 * 9 - 1)) == capi.OSH_ERR_INVALID and "stride is under 4 * cols" in capi.last_error(lib)
    if lib.osh_device_count() > 0:
        return                       # what follows covers the container without a GPU
    assert rc() == capi.OSH_ERR_NO_DEVICE and "device" in capi.last_error(lib).lower()


def test_libraries_export_the_new_entries():
    out = subprocess.run(["nm", "-DC", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("osh_orb_prepare", "osh_orb_extract_raw", "osh_orb_prepare_get_times", "osh_rectify_map_create", "osh_rectify_map_destroy"):
        assert name in out, name
    assert "ORB_SLAM3::" not in out and "osh::" not in out
    host = subprocess.run(["nm", "-DC", str(capi.HOST_LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "osh_host_orb_prepare_cpu" in host


def test_prepare_check_runs_clean_under_the_sanitizers():
    """make prepare-check: csrc/orb_prepare.h in a stand-alone host program under AddressSanitizer and UBSan."""
    r = subprocess.run(["make", "-C", str(CSRC), "prepare-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "prepare_check:" in r.stdout and "ERROR" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
