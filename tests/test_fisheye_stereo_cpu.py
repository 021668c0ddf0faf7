"""Frame::ComputeStereoFishEyeMatches without a device: the numpy restatement (tests/fisheye_stereo_numpy.py) on known-answer pairs,
a census of the committed generator cases by the restatement alone, the two float64 routes to the singular vector, the refusals of
osh_orb_fisheye_stereo_match / osh_kb8_triangulate (made before a context is looked at) and the export list."""
import ctypes as C
import dataclasses
import functools
import math
import subprocess

import numpy as np
import pytest

import fisheye_stereo_numpy as fn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_fisheye as sf

F = np.float32
KNOWN_PAIRS, PLAIN, PLAIN_RIG = fn.KNOWN_PAIRS, fn.PLAIN, fn.PLAIN_RIG


@functools.lru_cache(maxsize=None)
def case(name):
    fr = sf.make_fisheye_frame(**dict(fn.CASES)[name])
    return fr, fn.compute(fr)


@pytest.mark.parametrize("name", list(KNOWN_PAIRS))
def test_restatement_known_answers(name):
    p1, p2, ret, X = KNOWN_PAIRS[name]
    got, x3D, cosp, _ = fn.triangulate(PLAIN_RIG, p1, p2, 1.0, 1.0)
    if ret is not None:
        assert float(got) == ret
        assert (name != "identical_rays") or float(cosp) == 1.0
    else:
        # float32 rays (2^-24 relative each) through a triangulation with a parallax of 0.1 rad: 1e-5 covers it a hundred times
        assert got == x3D[2] and np.allclose(x3D, X, rtol=1e-5, atol=1e-6)


def test_unproject_inverts_project():
    cam = sf.CAM1
    for X in [(0.3, -0.2, 1.0), (-1.0, 0.4, 0.5), (0.0, 0.0, 2.0), (0.01, 0.02, 3.0)]:
        u, v = fn.project(cam, np.array(X, F))
        r = fn.unproject(cam, 1e-6, u, v)
        assert np.allclose([r[0], r[1]], [X[0] / X[2], X[1] / X[2]], rtol=2e-5, atol=2e-6)   # Newton stops at 1e-6 rad


@pytest.mark.parametrize("name", [n for n, _ in fn.CASES])
def test_few_borderline_matches_in_every_case(name):
    _, e = case(name)
    ok = e["ratio_ok"]
    assert e["borderline"][ok].sum() <= 0.02 * max(ok.sum(), 1), (int(e["borderline"][ok].sum()), int(ok.sum()))
    assert not e["borderline"][~ok].any()


def test_cases_reach_every_stage_and_share_right_keypoints():
    total = np.zeros(10, np.int64)
    shared = 0
    for name, _ in fn.CASES:
        _, e = case(name)
        total += np.bincount(e["stage"], minlength=10)
        l2r = e["left_to_right"]
        shared += int((np.bincount(l2r[l2r >= 0], minlength=1) >= 2).sum())
        assert np.array_equal(e["right_to_left"], fn.right_to_left_of(l2r, e["right_to_left"].shape[0]))
    assert (total >= 10).all(), total
    assert shared >= 1


@pytest.mark.parametrize("name", [n for n, _ in fn.CASES])
def test_two_float64_routes_give_adjacent_points(name):
    """svd of A against eigh of A^T A: x3D equal or adjacent in float32 wherever both accept, the same stage off the borderline."""
    fr, a = case(name)
    b = fn.compute(fr, route="eigh")
    firm = ~a["borderline"]
    assert np.array_equal(a["stage"][firm], b["stage"][firm])
    both = (a["stage"] == capi.OSH_FSTEREO_ACCEPTED) & (b["stage"] == capi.OSH_FSTEREO_ACCEPTED)
    if both.any():
        assert fn.ulp_distance(a["p3d"][both], b["p3d"][both]).max() <= 1
        assert fn.ulp_distance(a["depth"][both], b["depth"][both]).max() <= 1


def _refused(lib, fr, needle, results=True):
    cf, cr, _keep, _ = orb.fisheye_stereo_args([fr])
    rc = lib.osh_orb_fisheye_stereo_match(None, 1, cf, cr if results else None)
    assert rc == capi.OSH_ERR_INVALID, rc
    assert needle in capi.last_error(lib), capi.last_error(lib)


def test_refusals_need_no_device():
    lib = capi.load_library()
    fr = sf.make_fisheye_frame(11, n_left=50, n_right=40, mono_left=5, mono_right=4)
    rep = dataclasses.replace
    _refused(lib, rep(fr, mono_left=-1), "mono_left")
    _refused(lib, rep(fr, mono_left=51), "mono_left")
    _refused(lib, rep(fr, mono_right=41), "mono_right")
    _refused(lib, rep(fr, mono_right=-2), "mono_right")
    _refused(lib, rep(fr, left_octave=np.where(np.arange(50) == 7, 8, fr.left_octave).astype(np.int32)), "left octave")
    _refused(lib, rep(fr, right_octave=np.where(np.arange(40) == 3, -1, fr.right_octave).astype(np.int32)), "right octave")
    xy = fr.right_xy.copy(); xy[9, 1] = np.inf
    _refused(lib, rep(fr, right_xy=xy), "coordinate")
    cam = fr.cam2.copy(); cam[5] = np.nan
    _refused(lib, rep(fr, cam2=cam), "not finite")
    _refused(lib, rep(fr, precision1=float("nan")), "not finite")
    t = fr.tlr.copy(); t[0] = -np.inf
    _refused(lib, rep(fr, tlr=t), "not finite")
    sig = fr.level_sigma2.copy(); sig[2] = np.nan
    _refused(lib, rep(fr, level_sigma2=sig), "level_sigma2")
    cf, cr, _keep, _ = orb.fisheye_stereo_args([fr])
    cf[0].left_desc = C.cast(None, capi.c_uint8_p)
    assert lib.osh_orb_fisheye_stereo_match(None, 1, cf, cr) == capi.OSH_ERR_INVALID and "NULL" in capi.last_error(lib)
    cf, cr, _keep, _ = orb.fisheye_stereo_args([fr])
    cr[0].right_to_left = C.cast(None, capi.c_int32_p)
    assert lib.osh_orb_fisheye_stereo_match(None, 1, cf, cr) == capi.OSH_ERR_INVALID and "NULL" in capi.last_error(lib)
    # a well-formed frame gets as far as the missing context
    cf, cr, _keep, _ = orb.fisheye_stereo_args([fr])
    assert lib.osh_orb_fisheye_stereo_match(None, 1, cf, cr) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
    # osh_kb8_triangulate
    a = orb.kb8_pairs([[1, 2]], [[3, 4]], [1], [1])
    out = np.zeros(1, F)
    args = lambda rig, arrs: (None, 1, C.byref(rig), *[capi.ptr(x, capi.c_float_p) for x in arrs], capi.ptr(out, capi.c_float_p), None, None)
    bad = orb.kb8_rig(PLAIN, PLAIN, 1e-6, 1e-6, np.eye(3), [np.nan, 0, 0])
    assert lib.osh_kb8_triangulate(*args(bad, a)) == capi.OSH_ERR_INVALID and "not finite" in capi.last_error(lib)
    good = orb.kb8_rig(*PLAIN_RIG)
    nan_xy = orb.kb8_pairs([[np.nan, 2]], [[3, 4]], [1], [1])
    assert lib.osh_kb8_triangulate(*args(good, nan_xy)) == capi.OSH_ERR_INVALID and "not finite" in capi.last_error(lib)
    assert lib.osh_kb8_triangulate(None, 1, C.byref(good), None, None, None, None, None, None, None) == capi.OSH_ERR_INVALID
    assert "NULL" in capi.last_error(lib)
    assert lib.osh_kb8_triangulate(*args(good, a)) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)


def test_device_triangulation_compiled_for_the_host_equals_the_restatement():
    """csrc/kb8_triangulate.h, the statements the kernels run, on the host: return value and cosParallaxRays bit for bit, the point
    equal or adjacent in float32 (its singular vector comes from a Jacobi method, the restatement's from LAPACK)."""
    host = capi.load_host_library()
    for name in ("ahead", "behind"):
        fr, e = case(name)
        idx = np.nonzero(e["ratio_ok"])[0]
        r = e["best_right"][idx]
        a = orb.kb8_pairs(fr.left_xy[idx], fr.right_xy[r], fr.level_sigma2[fr.left_octave[idx]], fr.level_sigma2[fr.right_octave[r]])
        n = idx.size
        ret, p3d, cosp = np.zeros(n, F), np.zeros((n, 3), F), np.zeros(n, F)
        rig = orb.kb8_rig(*fn.rig_of(fr))
        assert host.osh_host_kb8_triangulate_cpu(n, C.byref(rig), *[capi.ptr(x, capi.c_float_p) for x in a], capi.ptr(ret, capi.c_float_p),
                                                 capi.ptr(p3d, capi.c_float_p), capi.ptr(cosp, capi.c_float_p)) == 0
        assert np.array_equal(cosp.view(np.uint32), e["cos_parallax"][idx].view(np.uint32))
        firm = ~e["borderline"][idx]
        acc = e["stage"][idx] == capi.OSH_FSTEREO_ACCEPTED
        assert np.array_equal((ret > F(0.0001))[firm], acc[firm])
        both = acc & (ret > F(0.0001))
        assert fn.ulp_distance(ret[both], e["depth"][idx][both]).max() <= 1
        assert fn.ulp_distance(p3d[both], e["p3d"][idx][both]).max() <= 1


def test_kernel_library_exports_the_fisheye_entries_and_no_cpp_symbols():
    out = subprocess.run(["nm", "-DC", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "osh_orb_fisheye_stereo_match" in out and "osh_kb8_triangulate" in out
    assert "ORB_SLAM3::" not in out
