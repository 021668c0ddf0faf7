"""The blur and the steered-BRIEF descriptors of ORBextractor::operator() without a GPU: the host build of csrc/orb_brief.h (the
statements the kernels run) against the numpy restatement of tests/brief_numpy.py bit for bit, the default weights, a census of
what the committed cases hold, the margin of every committed angle from a float32 rounding boundary, the refusals of
osh_orb_describe, which need no device, and the sanitizer program."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import brief_numpy as bn
from orb_slam3_study_kr_amd import capi, orb

F = np.float32
CSRC = capi.LIB_PATH.parent


@pytest.mark.parametrize("name", bn.CASE_NAMES)
def test_host_build_equals_the_restatement(name):
    it, exp = bn.case(name)
    for border in (0, 5):      # 5: levels as views into larger images, rows `stride` apart
        got, _ = orb.describe_cpu([it], borders=[border], debug=True)
        bn.assert_same(got[0], exp, f"{name} border {border}")


def test_host_build_on_a_large_frame():
    it, exp = bn.case("vga_752x480_L8")
    got, _ = orb.describe_cpu([it], borders=[19], debug=True)
    bn.assert_same(got[0], exp, "752x480")
    assert len(exp["descriptors"]) > 1000


def test_default_weights():
    w = orb.brief_gaussian_q8(7, 2.0)
    assert w.tolist() == [18, 34, 48, 56, 48, 34, 18] and int(w.sum()) == 256
    assert bn.default_weights().tolist() == w.tolist()
    for ksize, sigma in ((3, 0.8), (5, 1.1), (7, 1.0), (9, 2.5)):
        w = orb.brief_gaussian_q8(ksize, sigma)
        assert int(w.sum()) == 256 and w.tolist() == w[::-1].tolist() and w.tolist() == bn.default_weights(ksize, sigma).tolist()


def test_reach():
    assert orb.brief_reach(bn.seeded_table(1)) == bn.reach(bn.seeded_table(1)) == 19
    assert orb.brief_reach(bn.case("reach_22")[0]["pattern"]) == 22
    assert orb.brief_reach(np.zeros((512, 2), np.int8)) == 0
    t = np.zeros((512, 2), np.int8)
    t[5] = (3, 4)
    assert orb.brief_reach(t) == 5
    t[6] = (3, 5)      # sqrt(34) = 5.83
    assert orb.brief_reach(t) == 6
    # the stand-in constructor's table: its own, 512 points in [-13, 12]^2, reach 19
    p = orb.standin_pattern()
    assert p.shape == (512, 2) and p.min() == -13 and p.max() == 12 and orb.brief_reach(p) == 19 and len({tuple(q) for q in p.tolist()}) > 300


def test_census_of_the_committed_cases():
    """The restatement alone shows that the committed cases hold everything a kernel can get wrong."""
    # reflection in all four corners and on all four edges: the blurred pixel there differs from what a clamped border would give
    it, exp = bn.case("extremes_45x52")
    img, B = it["pyramid"][0], exp["blurred"][0]
    w = bn.default_weights()
    p = np.pad(img.astype(np.int64), ((0, 0), (3, 3)), mode="edge")
    h = sum(w[u] * p[:, u:u + img.shape[1]] for u in range(7))
    p = np.pad(h, ((3, 3), (0, 0)), mode="edge")
    clamped = ((sum(w[v] * p[v:v + img.shape[0], :] for v in range(7)) + 32768) >> 16).astype(np.uint8)
    diff = B != clamped
    assert not diff[3:-3, 3:-3].any()
    for region in (diff[:3, :3], diff[:3, -3:], diff[-3:, :3], diff[-3:, -3:], diff[:3, 3:-3], diff[-3:, 3:-3], diff[3:-3, :3], diff[3:-3, -3:]):
        assert region.any()
    # constant levels blur to themselves; the checkerboard (the largest differences) does not, and stays in range
    assert (bn.case("const_255")[1]["blurred"][0] == 255).all() and (bn.case("const_0")[1]["blurred"][0] == 0).all()
    assert (bn.case("const_255")[1]["descriptors"] == 0).all()
    cb = bn.case("checker")[1]["blurred"][0]
    assert 100 < cb.min() and cb.max() < 156 and len(np.unique(cb)) > 1
    # keypoints 19 pixels from each edge with the point of radius 18.38 turned onto that edge: a sample one pixel from it
    it, exp = bn.case("edges_60x70")
    cx, cy = it["xy"][:, 0].astype(int), it["xy"][:, 1].astype(int)
    assert math.hypot(*it["pattern"][0]) > 18
    assert cx[0] + exp["dx"][0, 0] == 1 and cx[1] + exp["dx"][1, 0] == 70 - 2 and cy[2] + exp["dy"][2, 0] == 1 and cy[3] + exp["dy"][3, 0] == 60 - 2
    # offsets exactly on k + 0.5, even and odd k, at 30 degrees (b == 0.5f); at 60 degrees a is 0.49999997f and rounds down
    it, exp = bn.case("extremes_45x52")
    t = it["pattern"].astype(np.int64)
    k30 = int(np.argwhere(it["angle"] == 30).ravel()[0])
    k60 = int(np.argwhere(it["angle"] == 60).ravel()[0])
    assert exp["cos_sin"][k30, 1] == F(0.5) and exp["cos_sin"][k60, 0] == F(0.49999997) and exp["cos_sin"][k60, 0] < F(0.5)
    halves = {}
    for j in np.argwhere((t[:, 1] == 0) & (t[:, 0] % 2 == 1)).ravel():
        halves[int(t[j, 0])] = int(exp["dy"][k30, j])
    assert halves[1] == 0 and halves[3] == 2 and halves[5] == 2 and halves[7] == 4 and halves[-1] == 0 and halves[-3] == -2      # ties to even
    down = {int(t[j, 0]): int(exp["dx"][k60, j]) for j in np.argwhere((t[:, 1] == 0) & (t[:, 0] % 2 == 1)).ravel()}
    assert down[1] == 0 and down[3] == 1 and down[5] == 2 and down[7] == 3 and down[-3] == -1
    # a fused multiply-add would land on another pixel
    for n_case, (angle, (px, py)) in enumerate(bn.FMA_CASES):
        k = int(np.argwhere(it["angle"] == angle).ravel()[0])
        j = int(np.argwhere((t[:, 0] == px) & (t[:, 1] == py)).ravel()[0])
        a, b = (np.float64(v) for v in exp["cos_sin"][k])
        unfused = int(exp["dx"][k, j])
        fused_first = int(np.rint(F(px * a - np.float64(F(F(py) * F(b))))))       # fma(px, a, -(py * b)): px * a exact in float64
        fused_second = int(np.rint(F(np.float64(F(F(px) * F(a))) - py * b)))      # fma(-py, b, px * a)
        assert unfused != fused_first, (angle, px, py, unfused, fused_first, fused_second)
        if n_case == 0:      # this one under either contraction
            assert unfused != fused_second, (angle, px, py, unfused, fused_first, fused_second)
    # equal samples give bit 0; both outcomes of the comparison occur
    j = 9       # points 18 and 19 are equal
    assert (t[18] == t[19]).all() and not (exp["descriptors"][:, 1] >> 1 & 1).any() and (exp["samples"][:, 18] == exp["samples"][:, 19]).all()
    allc = [bn.case(n) for n in bn.CASE_NAMES]
    ties = sum(int((e["samples"][:, 0::2] == e["samples"][:, 1::2]).sum()) for _, e in allc)
    ones = sum(int(np.unpackbits(e["descriptors"]).sum()) for _, e in allc)
    total = sum(e["descriptors"].size * 8 for _, e in allc)
    assert ties > 500 and 0.3 < ones / total < 0.6
    # angles in all four quadrants, and on the axes
    angles = np.concatenate([i["angle"] for i, _ in allc])
    assert {0.0, 90.0, 180.0, 270.0} <= set(angles.tolist())
    assert all(((angles > q) & (angles < q + 90)).sum() > 20 for q in (0, 90, 180, 270))
    # halves of the keypoint coordinates themselves, on the extreme positions
    assert any(((i["xy"] % 1) != 0).any() for i, _ in allc)


def test_committed_angles_are_far_from_float32_rounding_boundaries():
    """In np.longdouble: for every committed angle the exact cos(rad) and sin(rad) lie further than 2^-40 (relative) from the
    midpoint of two neighbouring float32 values, so every FP64 library with an error below 1 ulp (2^-52 relative) rounds to the
    same a and b: the device's, glibc's and numpy's must agree."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 here: the margins cannot be measured"
    angles = np.unique(np.concatenate([bn.case(n)[0]["angle"] for n in bn.CASE_NAMES + ["vga_752x480_L8"]]))
    rad = (angles * bn.FACTOR_PI).astype(F).astype(np.longdouble)
    worst = np.inf
    for fn in (np.cos, np.sin):
        v = fn(rad)
        f = v.astype(F)
        assert np.array_equal(f, fn(rad.astype(np.float64)).astype(F))
        for other in (np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))):
            mid = (f.astype(np.longdouble) + other.astype(np.longdouble)) / 2
            nz = v != 0
            margin = np.abs((v[nz] - mid[nz]) / v[nz])
            worst = min(worst, float(margin.min()))
    assert worst > 2.0 ** -40, worst


def _rc(lib, it, debug=False):
    cf, cr, _keep, _ = orb.describe_args([it], None, debug)
    return lib.osh_orb_describe(None, 1, cf, cr)


def test_refusals_need_no_device():
    lib = capi.load_library()
    base = bn.item("extremes_45x52")
    rows, cols = base["pyramid"][0].shape

    def refused(rc, needle, code=capi.OSH_ERR_INVALID):
        assert rc == code, (rc, needle, capi.last_error(lib))
        assert needle in capi.last_error(lib), (needle, capi.last_error(lib))

    def one(x, y, angle=10.0, level=0, **kw):
        return dict(base, xy=np.asarray([[20, 20], [x, y]], F), level=np.asarray([0, level], np.int32), angle=np.asarray([0, angle], F), **kw)

    # pyramids, as osh_orb_ic_angle
    refused(_rc(lib, dict(base, pyramid=base["pyramid"] * 17)), "n_levels 17 outside [1, 16]")
    refused(_rc(lib, dict(base, pyramid=(base["pyramid"][0], None))), "level 1 is NULL, empty or has stride < cols")
    cf, cr, _keep, _ = orb.describe_args([base])
    cf[0].pyramid[0].stride = cols - 1
    refused(lib.osh_orb_describe(None, 1, cf, cr), "level 0 is NULL, empty or has stride < cols")
    cf, cr, _keep, _ = orb.describe_args([base])
    cf[0].pyramid[0].rows = capi.OSH_FAST_MAX_SIDE + 1
    refused(lib.osh_orb_describe(None, 1, cf, cr), "exceeds", capi.OSH_ERR_UNSUPPORTED)
    # counts and arrays
    for field, needle in (("xy", "NULL keypoint array"), ("level", "NULL keypoint array"), ("angle", "NULL keypoint array")):
        cf, cr, _keep, _ = orb.describe_args([base])
        setattr(cf[0], field, C.cast(None, type(getattr(cf[0], field))))
        refused(lib.osh_orb_describe(None, 1, cf, cr), needle)
    cf, cr, _keep, _ = orb.describe_args([base])
    cr[0].descriptors = C.cast(None, capi.c_uint8_p)
    refused(lib.osh_orb_describe(None, 1, cf, cr), "NULL descriptors")
    cf, cr, _keep, _ = orb.describe_args([base])
    cf[0].n = -1
    refused(lib.osh_orb_describe(None, 1, cf, cr), "negative keypoint count")
    refused(lib.osh_orb_describe(None, 1, None, None), "bad arguments")
    refused(lib.osh_orb_describe(None, -1, None, None), "bad arguments")
    # the table
    refused(_rc(lib, dict(base, pattern=None)), "NULL pattern")
    for v in (16, -16, 127, -128):
        t = base["pattern"].copy()
        t[300, 1] = v
        refused(_rc(lib, dict(base, pattern=t)), "table point 300 outside [-15, 15]")
    # the weights
    for w in ([18, 34, 48, 56, 48, 34, 19], [0] * 7, [256, 0, 0, 0, 0, 0, 1], [65535, 257, 0, 0, 0, 0, 0]):
        refused(_rc(lib, dict(base, blur_q8=np.asarray(w, np.uint16))), "not 256")
    # keypoints
    refused(_rc(lib, one(np.nan, 20)), "keypoint 1 is not finite")
    refused(_rc(lib, one(20, np.inf)), "keypoint 1 is not finite")
    refused(_rc(lib, one(20, 20, angle=np.nan)), "keypoint 1 is not finite")
    refused(_rc(lib, one(20, 20, angle=-np.inf)), "keypoint 1 is not finite")
    refused(_rc(lib, one(20, 20, level=1)), "level 1 outside [0, 1)")
    refused(_rc(lib, one(20, 20, level=-1)), "level -1 outside")
    for x, y in ((18.4, 20), (20, 18.5), (cols - 19.4, 20), (20, rows - 19.4), (-1e30, 20), (1e30, 20), (20, 3e9), (-0.0, 20)):
        refused(_rc(lib, one(x, y)), "keypoint 1: the 39-pixel square leaves level 0")
    # the reach follows the table: with one point at (15, -15) the same keypoints need 22 pixels
    t = base["pattern"].copy()
    t[511] = (15, -15)
    refused(_rc(lib, one(21, 22, pattern=t)), "keypoint 0: the 45-pixel square leaves level 0")
    # a level too small for the blur cannot hold a keypoint even for a table of reach 0, and cannot be exported
    zero = np.zeros((512, 2), np.int8)
    small = dict(pyramid=(np.zeros((3, 50), np.uint8),), xy=np.asarray([[10, 1]], F), level=np.zeros(1, np.int32), angle=np.zeros(1, F), pattern=zero, blur_q8=None)
    refused(_rc(lib, small), "the 1-pixel square leaves level 0")
    empty = dict(small, xy=np.zeros((0, 2), F), level=np.zeros(0, np.int32), angle=np.zeros(0, F))
    refused(_rc(lib, empty, debug=True), "fewer than 4 rows or columns", capi.OSH_ERR_UNSUPPORTED)
    # halves go to the even pixel: 18.5 -> 18 is outside, 19.5 -> 20 and cols - 20.5 -> cols - 20 are inside, as far as the missing context
    refused(_rc(lib, one(19.5, 19.0)), "no context")
    refused(_rc(lib, one(cols - 20.5, rows - 20.0)), "no context")
    refused(_rc(lib, base), "no context")
    refused(_rc(lib, empty), "no context")
    refused(_rc(lib, dict(base, blur_q8=np.asarray([0, 0, 0, 256, 0, 0, 0], np.uint16))), "no context")
    # a token can only be looked up on a context
    refused(_rc(lib, dict(base, pyramid=None, token=5)), "no context")


def test_libraries_export_the_new_entries():
    out = subprocess.run(["nm", "-DC", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("osh_orb_describe", "osh_orb_describe_get_times"):
        assert name in out, name
    assert "ORB_SLAM3::" not in out and "osh::" not in out
    host = subprocess.run(["nm", "-DC", str(capi.HOST_LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("osh_host_orb_describe_cpu", "osh_host_orbextractor_extract", "ORB_SLAM3::ORBextractor::operator()", "ORB_SLAM3::ORBextractor::ComputePyramid"):
        assert name in host, name


def test_brief_check_runs_clean_under_the_sanitizers():
    """make brief-check: csrc/orb_brief.h in a stand-alone host program under AddressSanitizer and UBSan."""
    r = subprocess.run(["make", "-C", str(CSRC), "brief-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "brief_check:" in r.stdout and "ERROR" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
