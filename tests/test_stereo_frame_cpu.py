"""The calls that extract and match a rectified stereo frame, without a device: the census of the named pairs through the chain of
the CPU restatements (pyramid, detector, quadtree, IC_Angle, descriptors, level-0 scaling, stereo_numpy); the refusals of
osh_orb_stereo_match_resident and osh_orb_extract_stereo that need no context; and `make stereo-frame-check`, the host half
(validation, token checks and the level plan from a PyramidTable) under AddressSanitizer and UBSan."""
import functools
import subprocess

import numpy as np
import pytest

import stereo_frame_cases as sc
import stereo_numpy as sn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_stereo as ss

F = np.float32


@functools.lru_cache(maxsize=None)
def _cpu_frame(name):
    p = sc.pair(name)
    left, right = sc.extract_cpu(p["left"]), sc.extract_cpu(p["right"])
    return sc.stereo_frame(p, left, right, left["levels"], right["levels"])


@pytest.mark.parametrize("name", sc.PAIR_NAMES)
def test_every_named_pair_meets_the_census(name):
    fr = _cpu_frame(name)
    out = sn.compute_stereo_matches(fr)
    print(name, "left", len(fr.left_octave), "right", len(fr.right_octave), "stages", np.bincount(out["stage"], minlength=9).tolist())
    sc.assert_census(out["stage"], fr.left_octave, name)


def test_the_level0_scaling_is_one_float32_multiply_and_leaves_level_0_alone():
    xy = np.array([[16.5, 20.25], [100.0, 33.0], [19.0, 19.0]], F)
    s = sc.scales(3)
    got = sc.level0(xy, np.array([0, 2, 1], np.int32), s)
    assert np.array_equal(got[0], xy[0])
    assert got[1, 0] == F(F(100.0) * s[2]) and got[1, 1] == F(F(33.0) * s[2]) and got[2, 0] == F(F(19.0) * s[1])


# ---------------------------------------------------------------------------------------------- refusals: no context, no device
def _resident_frame(**change):
    fr = ss.make_shift_frame(1, 4, n=12)[0]
    for k, v in change.items():
        setattr(fr, k, v)
    return fr


def _refused_resident(lib, fr, needle, code=capi.OSH_ERR_INVALID, tokens=(1, 2), null_out=False):
    cf, cr, _keep, _outs = orb.stereo_resident_args([fr], [tokens])
    if null_out:
        cr[0].u_right = None
    assert lib.osh_orb_stereo_match_resident(None, 1, cf, cr) == code, needle
    assert needle in capi.last_error(lib), (needle, capi.last_error(lib))


def test_the_resident_stage_refuses_without_a_context_what_the_stage_refuses():
    lib = capi.load_library()
    base = _resident_frame()
    _refused_resident(lib, base, "no context")                                       # everything else passed
    _refused_resident(lib, _resident_frame(b=0.0), "bad bf / b")
    _refused_resident(lib, _resident_frame(bf=float("inf")), "bad bf / b")
    _refused_resident(lib, _resident_frame(b=float("nan")), "bad bf / b")
    bad = base.left_octave.copy(); bad[3] = base.n_levels
    _refused_resident(lib, _resident_frame(left_octave=bad), "left octave")
    bad = base.right_octave.copy(); bad[0] = -1
    _refused_resident(lib, _resident_frame(right_octave=bad), "right octave")
    bad = base.left_xy.copy(); bad[2, 1] = np.nan
    _refused_resident(lib, _resident_frame(left_xy=bad), "coordinate not finite")
    bad = base.right_xy.copy(); bad[1, 0] = 2.0e6
    _refused_resident(lib, _resident_frame(right_xy=bad), "coordinate not finite")
    _refused_resident(lib, base, "NULL left keypoint or result array", null_out=True)
    cf, cr, _keep, _outs = orb.stereo_resident_args([base], [(1, 2)])
    cf[0].n_levels = 17
    assert lib.osh_orb_stereo_match_resident(None, 1, cf, cr) == capi.OSH_ERR_INVALID and "n_levels 17" in capi.last_error(lib)
    cf[0].n_levels, cf[0].n_left = base.n_levels, -1
    assert lib.osh_orb_stereo_match_resident(None, 1, cf, cr) == capi.OSH_ERR_INVALID and "negative keypoint count" in capi.last_error(lib)
    cf[0].n_left, cf[0].scale_factors = len(base.left_octave), None
    assert lib.osh_orb_stereo_match_resident(None, 1, cf, cr) == capi.OSH_ERR_INVALID and "NULL scale factors" in capi.last_error(lib)
    assert lib.osh_orb_stereo_match_resident(None, 1, None, cr) == capi.OSH_ERR_INVALID and "bad arguments" in capi.last_error(lib)
    assert lib.osh_orb_stereo_match_resident(None, -1, cf, cr) == capi.OSH_ERR_INVALID


def _fused(lib, pairs, capacities, change=None, raw=False, **null):
    pf, cf, cp, cr, cs, _keep, _outs, _souts = orb.extract_stereo_args(pairs, capacities, stages=True, raw=raw)
    if change:
        change(cf, cp, cr, cs)
    rc = lib.osh_orb_extract_stereo(None, len(pairs), pf, cf, None if null.get("no_pairs") else cp, cr, None if null.get("no_results") else cs)
    return rc, capi.last_error(lib)


def test_the_fused_call_refuses_without_a_context_what_it_refuses():
    lib = capi.load_library()
    p = sc.pair("pair_160x120_L3")
    other = sc.custom_pair(p["left"]["image"], p["right"]["image"], 4, 300)
    ok = lambda rc, msg, needle, code=capi.OSH_ERR_INVALID: (rc == code and needle in msg) or pytest.fail(f"{needle!r}: rc {rc}, {msg!r}")
    ok(*_fused(lib, [p], [400, 400]), "no context")                                  # everything else passed
    ok(*_fused(lib, [p], [400, 400], raw=True), "no context")
    ok(*_fused(lib, [p], [400, 400], no_pairs=True), "NULL pairs or stereo_results")
    ok(*_fused(lib, [p], [400, 400], no_results=True), "NULL pairs or stereo_results")
    for bf, b in ((40.0, 0.0), (40.0, -1.0), (float("inf"), 1.0), (40.0, float("nan")), (float("nan"), 1.0)):
        ok(*_fused(lib, [dict(p, bf=bf, b=b)], [400, 400]), "bad bf / b")
    ok(*_fused(lib, [p, dict(p, b=0.0)], [400, 400, 400, 400]), "pair 1: bad bf / b")
    ok(*_fused(lib, [dict(p, right=other["right"])], [400, 400]), "the left frame has 3 levels, the right frame 4")

    def no_u_right(cf, cp, cr, cs):
        cs[0].u_right = None
    ok(*_fused(lib, [p], [400, 400], no_u_right), "NULL u_right or depth with a left capacity of 400")

    def no_depth(cf, cp, cr, cs):
        cs[0].depth = None
    ok(*_fused(lib, [p], [400, 400], no_depth), "NULL u_right or depth")
    ok(*_fused(lib, [p], [0, 400], no_depth), "no context")                           # no room on the left: nothing to point at

    # what osh_orb_extract refuses stays refused
    def bad_threshold(cf, cp, cr, cs):
        cf[1].min_th = 0
    rc, msg = _fused(lib, [p], [400, 400], bad_threshold)
    ok(rc, msg, "frame 1: threshold outside [1, 255]")
    rc = lib.osh_orb_extract_stereo(None, -1, None, None, None, None, None)
    assert rc == capi.OSH_ERR_INVALID and "bad arguments" in capi.last_error(lib)
    assert lib.osh_orb_extract_stereo(None, 40000, None, *orb.extract_stereo_args([p], [0, 0])[1:5]) == capi.OSH_ERR_UNSUPPORTED
    ms = np.zeros(5)
    assert lib.osh_orb_extract_stereo_get_times(None, capi.ptr(ms, capi.c_double_p)) == capi.OSH_ERR_INVALID


def test_make_stereo_frame_check_passes():
    run = subprocess.run(["make", "-C", str(capi.LIB_PATH.parent), "stereo-frame-check"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "stereo_frame_check ok" in run.stdout and "ERROR" not in run.stdout + run.stderr and "runtime error" not in run.stdout + run.stderr
