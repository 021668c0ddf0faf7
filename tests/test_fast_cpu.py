"""The integer part of ORBextractor::ComputeKeyPointsOctTree without a GPU: the host build of csrc/orb_fast.h (the statements the
kernels run) against the numpy restatement of tests/fast_numpy.py bit for bit, a census of what the committed seeds hold, the cell
geometry against a hand-computed table, and the refusals of osh_orb_fast_detect / osh_orb_ic_angle, which need no device."""
import ctypes as C
import dataclasses
import subprocess

import numpy as np
import pytest

import fast_numpy as fn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_fast as sf

F = np.float32


@pytest.mark.parametrize("name", fn.CASE_NAMES)
def test_host_build_equals_the_restatement(name):
    frame, exp, (kxy, klevel), exp_angle = fn.case(name)
    for border in (0, 5):      # 5: levels as views into larger images, rows `stride` apart
        got, _ = orb.fast_cpu([frame], borders=[border])
        assert got[0]["n_out"] == len(exp["level"]) and got[0]["n_cells"] == len(exp["used_min_th"])
        fn.assert_detect_same(got[0], exp, f"{name} border {border}")
        ang, _ = orb.ic_angle_cpu([dict(xy=kxy, level=klevel, pyramid=frame.pyramid)], borders=[border])
        fn.assert_angles_same(ang[0], exp_angle, f"{name} border {border}")


def test_host_build_on_the_moment_frame_and_a_large_frame():
    frame, xy, level = sf.moment_frame()
    exp = fn.ic_angle(frame.pyramid, xy, level)
    got, _ = orb.ic_angle_cpu([dict(xy=xy, level=level, pyramid=frame.pyramid)])
    fn.assert_angles_same(got[0], exp, "moment frame")
    # known answers: uniform block, ramps along x (up, down), along y (up, down)
    assert (got[0]["angle"][:4] == 0).all() and (got[0]["m10"][:4] == 0).all() and (got[0]["m01"][:4] == 0).all()
    assert got[0]["angle"][4:20].tolist() == [0.0] * 4 + [180.0] * 4 + [90.0] * 4 + [270.0] * 4
    frame, exp, (kxy, klevel), exp_angle = fn.case("vga_752x480_L8")
    fn.assert_detect_same(orb.fast_cpu([frame])[0][0], exp, "752x480")
    fn.assert_angles_same(orb.ic_angle_cpu([dict(xy=kxy, level=klevel, pyramid=frame.pyramid)])[0][0], exp_angle, "752x480")


def test_census_of_the_committed_seeds():
    """The restatement alone shows, over the committed cases, everything the kernels can get wrong.

    Item b of the issue asks for corners emitted by two cells of the overlap.  There are none, by construction: cell j has scores
    in columns [iniX + 3, iniX + wCell + 3) and cell j + 1 starts at iniX + wCell, so the scored areas of neighbouring cells tile
    the level and the 6-pixel overlap is exactly FAST's two 3-pixel rims.  The census therefore asserts that no pixel is emitted
    twice, and counts what the overlap does produce: adjacent pixels on either side of a cell edge that are both emitted, although
    the stronger would have suppressed the weaker in an undivided image (each lies in the other's score-free rim)."""
    used, scores_hit, pol, wrap, tie, twice, edge_pairs = np.zeros(3, int), [set(), set(), set(), set()], set(), 0, 0, 0, 0
    quadrants, branches = set(), set()
    for name in fn.CASE_NAMES:
        frame, exp, _, ang = fn.case(name)
        cs = exp["census"]
        used += np.bincount(exp["used_min_th"], minlength=3)
        for k, t in enumerate((frame.ini_th, frame.ini_th - 1, frame.min_th, frame.min_th - 1)):
            if t in cs["scores"]:
                scores_hit[k].add(name)
        pol |= cs["pol"]; wrap += cs["wrap"]; tie += cs["tie"]; twice += cs["twice"]; edge_pairs += cs["edge_pairs"]
        for a, b in zip(ang["m10"].tolist(), ang["m01"].tolist()):
            if a and b:
                quadrants.add((a > 0, b > 0))
            branches.add(abs(a) >= abs(b))
    frame, xy, level = sf.moment_frame()
    ang = fn.ic_angle(frame.pyramid, xy, level)
    zero10, zero01 = int(((ang["m10"] == 0) & (ang["m01"] != 0)).sum()), int(((ang["m01"] == 0) & (ang["m10"] != 0)).sum())
    assert used[capi.OSH_FAST_AT_INI] > 50 and used[capi.OSH_FAST_AT_MIN] >= 5 and used[capi.OSH_FAST_EMPTY] >= 5, used      # a
    assert twice == 0 and edge_pairs >= 10, (twice, edge_pairs)                                                            # b
    assert tie >= 100, tie                                                                                                 # c
    assert all(scores_hit), scores_hit                                                                                     # d
    assert pol == {1, -1} and wrap >= 100, (pol, wrap)                                                                     # e
    assert len(quadrants) == 4 and branches == {True, False} and zero10 >= 4 and zero01 >= 4                               # f
    assert (ang["m10"] > 0).any() and (ang["m10"] < 0).any() and (ang["m01"] > 0).any() and (ang["m01"] < 0).any()


# rows, cols -> nCols, nRows, wCell, hCell, maxBorderX, maxBorderY, existing cells, (x0, y0, w, h) of the last existing cell.  By hand:
# width = cols - 32, nCols = floor(width / 35), wCell = ceil(width / nCols); cell j starts at 16 + j * wCell, is cut at maxBorderX
# and is dropped when it starts at or after maxBorderX - 6 (rows: maxBorderY - 3).
GEOMETRY = [
    ((67, 67), (1, 1, 35, 35, 51, 51), 1, (16, 16, 35, 35)),
    ((67, 66), (0, 0, 0, 0, 50, 51), 0, None),                        # 34 columns between the borders: no cells
    ((66, 67), (0, 0, 0, 0, 51, 50), 0, None),
    # width 2101, nCols 60, wCell ceil(35.0167) = 36: cell 58 spans [2104, 2117), cell 59 would start at 2140 >= 2111
    ((67, 2133), (60, 1, 36, 35, 2117, 51), 59, (2104, 16, 13, 35)),
    # the twin: height 2101, hCell 36, cell 58 spans rows [2104, 2117); cell 59 starts at 2140 >= 2117 - 3
    ((2133, 67), (1, 60, 35, 36, 51, 2117), 59, (16, 2104, 35, 13)),
    # 752 x 480: width 720, nCols 20, wCell 36; height 448, nRows 12, hCell ceil(37.33) = 38; the last row of cells starts at
    # 16 + 11 * 38 = 434 < 461 and is cut to 30 rows, the last column at 16 + 19 * 36 = 700 < 730 to 36 columns
    ((480, 752), (20, 12, 36, 38, 736, 464), 240, (700, 434, 36, 30)),
    # 640 x 480: width 608, nCols 17, wCell ceil(35.76) = 36; the last column starts at 16 + 16 * 36 = 592 < 618, cut to 32
    ((480, 640), (17, 12, 36, 38, 624, 464), 204, (592, 434, 32, 30)),
]


@pytest.mark.parametrize("shape,geom,n_cells,last", GEOMETRY)
def test_geometry_table(shape, geom, n_cells, last):
    got, rects = orb.fast_level_cells(*shape)
    assert got == geom
    assert len(rects) == n_cells
    if last:
        assert tuple(rects[-1]) == last
    assert fn.geometry(*shape) == geom and [c[2:] for c in fn.cells(*shape)] == [tuple(r) for r in rects.tolist()]


def test_geometry_of_eight_level_pyramids():
    """Every level of the 752 x 480 and 640 x 480 pyramids at scale 1.2: the C-ABI's cells equal the restatement's, every cell
    lies inside its level and is at most 75 pixels wide and high."""
    for h, w in ((480, 752), (480, 640)):
        sizes = sf.level_sizes(h, w, 8)
        assert sizes[0] == (h, w) and sizes[7] == ((134, 210) if w == 752 else (134, 179))
        for rows, cols in sizes:
            got, rects = orb.fast_level_cells(rows, cols)
            assert got == fn.geometry(rows, cols) and [c[2:] for c in fn.cells(rows, cols)] == [tuple(r) for r in rects.tolist()]
            assert len(rects) and (rects[:, 0] >= 16).all() and (rects[:, 0] + rects[:, 2] <= cols - 16).all()
            assert (rects[:, 1] + rects[:, 3] <= rows - 16).all() and rects[:, 2:].max() <= 75 and rects[:, 2].min() >= 7


def _detect_rc(lib, frame, capacity=(10, 10)):
    cf, cr, _keep, _ = orb.fast_args([frame], [capacity])
    return lib.osh_orb_fast_detect(None, 1, cf, cr)


def test_refusals_need_no_device():
    lib = capi.load_library()
    frame = fn.case("mix_160x120")[0]
    rep = dataclasses.replace

    def refused(rc, needle, code=capi.OSH_ERR_INVALID):
        assert rc == code, (rc, needle, capi.last_error(lib))
        assert needle in capi.last_error(lib), (needle, capi.last_error(lib))

    # thresholds
    for ini, mn in ((0, 0), (256, 7), (20, 0), (20, -3)):
        refused(_detect_rc(lib, rep(frame, ini_th=ini, min_th=mn)), "threshold outside [1, 255]")
    refused(_detect_rc(lib, rep(frame, ini_th=7, min_th=8)), "min_th 8 > ini_th 7")
    # level counts, NULL and empty levels, stride < cols
    refused(_detect_rc(lib, rep(frame, pyramid=frame.pyramid[:1] * 17)), "n_levels 17 outside [1, 16]")
    cf, cr, _keep, _ = orb.fast_args([frame], [(10, 10)])
    cf[0].n_levels = 0
    refused(lib.osh_orb_fast_detect(None, 1, cf, cr), "n_levels 0 outside")
    refused(_detect_rc(lib, rep(frame, pyramid=(frame.pyramid[0], None, frame.pyramid[2]))), "level 1 is NULL, empty or has stride < cols")
    for field, value in (("rows", 0), ("cols", 0), ("stride", frame.pyramid[2].shape[1] - 1)):
        cf, cr, _keep, _ = orb.fast_args([frame], [(10, 10)])
        setattr(cf[0].pyramid[2], field, value)
        refused(lib.osh_orb_fast_detect(None, 1, cf, cr), "level 2 is NULL, empty or has stride < cols")
    cf, cr, _keep, _ = orb.fast_args([frame], [(10, 10)])
    cf[0].pyramid = C.cast(None, C.POINTER(capi.StereoImage))
    refused(lib.osh_orb_fast_detect(None, 1, cf, cr), "NULL pyramid")
    cf, cr, _keep, _ = orb.fast_args([frame], [(10, 10)])
    cf[0].pyramid[0].rows = capi.OSH_FAST_MAX_SIDE + 1
    refused(lib.osh_orb_fast_detect(None, 1, cf, cr), "exceeds", capi.OSH_ERR_UNSUPPORTED)
    # result arrays
    cf, cr, _keep, _ = orb.fast_args([frame], [(10, 10)])
    cr[0].capacity = -1
    refused(lib.osh_orb_fast_detect(None, 1, cf, cr), "negative capacity")
    cf, cr, _keep, _ = orb.fast_args([frame], [(10, 10)])
    cr[0].xy = C.cast(None, capi.c_float_p)
    refused(lib.osh_orb_fast_detect(None, 1, cf, cr), "NULL result array")
    cf, cr, _keep, _ = orb.fast_args([frame], [(10, 10)])
    cr[0].level_count = C.cast(None, capi.c_int32_p)
    refused(lib.osh_orb_fast_detect(None, 1, cf, cr), "NULL level_count")
    refused(lib.osh_orb_fast_detect(None, -1, None, None), "bad arguments")
    refused(lib.osh_orb_fast_detect(None, 1, None, None), "bad arguments")
    # well-formed calls get as far as the missing context
    refused(_detect_rc(lib, frame), "no context")
    refused(_detect_rc(lib, frame, (0, 0)), "no context")

    # IC_Angle: keypoints against the pyramid they come with
    h, w = frame.pyramid[1].shape

    def ic_rc(xy, level, pyramid=frame.pyramid):
        cf, cr, _keep, _ = orb.ic_angle_args([dict(xy=np.asarray(xy, F), level=np.asarray(level, np.int32), pyramid=pyramid)])
        return lib.osh_orb_ic_angle(None, 1, cf, cr)

    refused(ic_rc([[np.nan, 30]], [0]), "keypoint 0 is not finite")
    refused(ic_rc([[30, 30], [30, np.inf]], [0, 0]), "keypoint 1 is not finite")
    refused(ic_rc([[30, 30]], [3]), "level 3 outside [0, 3)")
    refused(ic_rc([[30, 30]], [-1]), "level -1 outside")
    for x, y in ((14.4, 30), (30, 14.5), (w - 15.5, 30), (30, h - 15.4), (-1e30, 30), (1e30, 30), (30, 3e9)):
        refused(ic_rc([[40, 40], [x, y]], [1, 1]), "keypoint 1: the 31-pixel disc leaves level 1")
    refused(ic_rc([[30, 30]], [0], pyramid=(frame.pyramid[0], None)), "level 1 is NULL")
    # halves go to the even pixel: 14.5 -> 14 is outside, 15.5 -> 16 and w - 16.5 -> w - 16 are inside, as far as the missing context
    refused(ic_rc([[15.5, 15.0], [w - 16.5, h - 16.0]], [1, 1]), "no context")
    cf, cr, _keep, _ = orb.ic_angle_args([dict(xy=np.zeros((1, 2), F) + 30, level=np.zeros(1, np.int32), pyramid=frame.pyramid)])
    cf[0].n = -2
    refused(lib.osh_orb_ic_angle(None, 1, cf, cr), "negative keypoint count")
    cf[0].n = 1
    cf[0].xy = C.cast(None, capi.c_float_p)
    refused(lib.osh_orb_ic_angle(None, 1, cf, cr), "NULL keypoint array")
    refused(lib.osh_orb_ic_angle(None, 1, None, None), "bad arguments")
    # a token can only be looked up on a context
    cf, cr, _keep, _ = orb.ic_angle_args([dict(xy=np.zeros((1, 2), F) + 30, level=np.zeros(1, np.int32), token=5)])
    refused(lib.osh_orb_ic_angle(None, 1, cf, cr), "no context")


def test_kernel_library_exports_the_new_entries_and_no_cpp_symbols():
    out = subprocess.run(["nm", "-DC", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("osh_orb_fast_detect", "osh_orb_ic_angle", "osh_orb_fast_get_times", "osh_orb_ic_angle_get_times"):
        assert name in out, name
    assert "ORB_SLAM3::" not in out and "osh::" not in out
    host = subprocess.run(["nm", "-DC", str(capi.HOST_LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("osh_host_orb_fast_cpu", "osh_host_orb_ic_angle_cpu", "osh_host_orb_fast_level_cells", "osh_host_orbextractor_compute_keypoints",
                 "ORB_SLAM3::ORBextractor::ComputeKeyPointsOctTree"):
        assert name in host, name
