"""The per-match body of LocalMapping::CreateNewMapPoints without a device: the host build of csrc/newpoint_triangulate.h (the
statements k_newpoint_triangulate runs) against the numpy restatement (tests/newpoints_numpy.py), a census of the committed
generator cases by the restatement alone, known answers, the refusals of osh_orb_triangulate_new_points (made before a context is
looked at) and the export list."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

import newpoints_numpy as nn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_newpoints as sn

F = np.float32
NAMES = [n for n, _ in nn.CASES]


@functools.lru_cache(maxsize=None)
def case(name):
    seg = sn.make_segment(**dict(nn.CASES)[name])
    return seg, nn.compute(seg)


@pytest.mark.parametrize("name", NAMES)
def test_host_build_of_the_header_equals_the_restatement(name):
    """Stage, source and cosParallaxRays bit for bit off the borderline; x3D of the accepted pairs in every bit (the Jacobi null
    vector against LAPACK's: both FP64, rounded to float32 once)."""
    seg, e = case(name)
    got = orb.newpoint_cpu([seg])[0][0]
    nn.assert_matches(got, e, name, x3d_ulp=0)


@pytest.mark.parametrize("name", NAMES)
def test_few_borderline_pairs_in_every_case(name):
    _, e = case(name)
    assert e["borderline"].sum() <= 0.02 * e["borderline"].size, (int(e["borderline"].sum()), e["borderline"].size)


def test_cases_reach_every_stage_source_and_branch():
    stages, sources, branches = np.zeros(11, np.int64), np.zeros(3, np.int64), {}
    for name in NAMES:
        _, e = case(name)
        stages += np.bincount(e["stage"], minlength=11)
        sources += np.bincount(e["source"][e["source"] != capi.OSH_NEWPOINT_NO_SOURCE], minlength=3)
        for rec in e["branches"]:
            for b in rec:
                branches[b] = branches.get(b, 0) + 1
    assert (stages >= 10).all(), stages
    assert (sources >= 10).all(), sources
    for b in ("rig_LL", "rig_LR", "rig_RL", "rig_RR", "cos_stereo1", "cos_stereo2", "triangulate", "stereo1", "stereo2", "mono_reproj", "stereo_reproj"):
        assert branches.get(b, 0) >= 10, (b, branches)
    # the accepted points of the stereo cases come from all three sources
    for name in ("stereo", "stereo_inertial_far"):
        _, e = case(name)
        acc = e["stage"] == capi.OSH_NEWPOINT_ACCEPTED
        assert (np.bincount(e["source"][acc], minlength=3)[:3] >= 10).all(), name


def test_inertial_and_far_point_switches_change_the_outcome():
    seg, e = case("mono")
    far = nn.compute(dataclasses.replace(seg, far_points=True, th_far_points=3.2))
    assert (far["stage"] == capi.OSH_NEWPOINT_FAR).sum() >= 10 and not (e["stage"] == capi.OSH_NEWPOINT_FAR).any()
    # a cosine between the two limits: triangulated without an IMU, given up with one
    mid = sn.make_segment(21, "mono", 40, outliers=0.0, low=0.0)
    k2 = mid.kf2
    Ow = (mid.kf1.pose.Ow + F(0.02) * mid.kf1.pose.Rwc[:, 0]).astype(F)     # 2 cm to the side of the current keyframe
    pose = sn.Pose(mid.kf1.pose.Rcw, (-(mid.kf1.pose.Rcw @ Ow)).astype(F), mid.kf1.pose.Rwc, Ow)
    pts = []
    for i in range(mid.n):
        xn = nn.unproject(mid.kf1.camera, mid.pt1[i, 0], mid.pt1[i, 1])
        X = mid.kf1.pose.Rwc.astype(np.float64) @ (np.array(xn, np.float64) * 0.82) + mid.kf1.pose.Ow    # parallax about 0.0244 rad
        pts.append(sn.project(k2.camera, pose.Rcw.astype(np.float64) @ X + pose.tcw))
    mid = dataclasses.replace(mid, kf2=dataclasses.replace(k2, pose=pose), pt2=np.asarray(pts, F))
    a, b = nn.compute(mid), nn.compute(dataclasses.replace(mid, inertial=True))
    between = (a["cos_parallax"].astype(np.float64) > 0.9996) & (a["cos_parallax"].astype(np.float64) < 0.9998)
    assert between.sum() >= 10
    assert (a["source"][between] == capi.OSH_NEWPOINT_TRIANGULATED).all() and (b["stage"][between] == capi.OSH_NEWPOINT_LOW_PARALLAX).all()
    for seg2, exp in ((mid, a), (dataclasses.replace(mid, inertial=True), b)):
        got = orb.newpoint_cpu([seg2])[0][0]
        assert np.array_equal(got["stage"][between], exp["stage"][between]) and np.array_equal(got["source"][between], exp["source"][between])


def test_known_answer_on_a_plain_pair():
    """Two axis-aligned pinhole keyframes 0.2 m apart looking at (0.1, 0, 2): the triangulated point is that point."""
    cam = sn.Camera(sn.PINHOLE, np.array([400, 400, 320, 240, 0, 0, 0, 0], F))
    k1 = sn._keyframe(sn.make_pose(np.eye(3), [0, 0, 0]), cam, 4)
    k2 = sn._keyframe(sn.make_pose(np.eye(3), [-0.2, 0, 0]), cam, 4)
    seg = sn._flat_segment(k1, k2, 1, (320 + 400 * 0.05, 240), (320 + 400 * (-0.05), 240))
    for r in (nn.compute(seg), orb.newpoint_cpu([seg])[0][0]):
        assert r["stage"][0] == capi.OSH_NEWPOINT_ACCEPTED and r["source"][0] == capi.OSH_NEWPOINT_TRIANGULATED
        # float32 rays through a parallax of 0.1 rad: 1e-5 covers 2^-24 a hundred times
        assert np.allclose(r["x3d"][0], [0.1, 0.0, 2.0], rtol=1e-5, atol=1e-6)


def test_quirks_of_the_reference_are_kept():
    seg, e = case("stereo")
    # cosParallaxStereo2 is only computed when bStereo1 is false
    both = (seg.u_right1 >= 0) & (seg.u_right2 >= 0)
    assert both.sum() >= 10
    assert all("cos_stereo2" not in e["branches"][i] for i in np.nonzero(both)[0])
    # the neighbour's stereo test subtracts the current keyframe's mbf: another mbf of the neighbour changes nothing,
    # another mbf of the current keyframe does
    other2 = dataclasses.replace(seg, kf2=dataclasses.replace(seg.kf2, mbf=seg.kf2.mbf * 2))
    nn.assert_same(orb.newpoint_cpu([other2])[0][0], orb.newpoint_cpu([seg])[0][0], "kf2.mbf")
    other1 = dataclasses.replace(seg, kf1=dataclasses.replace(seg.kf1, mbf=seg.kf1.mbf * 2))
    changed = orb.newpoint_cpu([other1])[0][0]["stage"]
    assert ((changed == capi.OSH_NEWPOINT_REPROJ_2) & (e["stage"] == capi.OSH_NEWPOINT_ACCEPTED) & (seg.u_right2 >= 0) & (seg.u_right1 < 0)).sum() >= 10
    # bStereo is false on a rig, whatever mvuRight says
    rig, er = case("rig")
    wet = dataclasses.replace(rig, u_right1=np.full(rig.n, 10, F), depth1=np.full(rig.n, 1, F))
    nn.assert_same(orb.newpoint_cpu([wet])[0][0], orb.newpoint_cpu([rig])[0][0], "rig mvuRight")
    assert (er["source"][er["source"] != capi.OSH_NEWPOINT_NO_SOURCE] == capi.OSH_NEWPOINT_TRIANGULATED).all()


def _call(lib, segs, results=True):
    cs, cr, _keep, _ = orb.newpoint_args(segs)
    return lib.osh_orb_triangulate_new_points(None, len(segs), cs, cr if results else None)


def _refused(lib, seg, needle, code=capi.OSH_ERR_INVALID):
    rc = _call(lib, [seg])
    assert rc == code, (rc, needle)
    assert needle in capi.last_error(lib), (needle, capi.last_error(lib))


def test_refusals_need_no_device():
    lib = capi.load_library()
    seg = case("rig")[0].head(20)
    st = case("stereo")[0].head(20)
    rep = dataclasses.replace

    def with_kf(s, which, **kw):
        return rep(s, **{which: rep(getattr(s, which), **kw)})

    def poked(a, at, value):
        a = a.copy(); a[at] = value
        return a

    # non-finite poses, keypoints or parameters
    p = seg.kf1.pose
    _refused(lib, with_kf(seg, "kf1", pose=rep(p, tcw=poked(p.tcw, 1, np.nan))), "pose entry not finite")
    pr = seg.kf2.right_pose
    _refused(lib, with_kf(seg, "kf2", right_pose=rep(pr, Rwc=poked(pr.Rwc, (1, 2), np.inf))), "right pose entry not finite")
    _refused(lib, with_kf(seg, "kf2", pose=rep(seg.kf2.pose, Ow=poked(seg.kf2.pose.Ow, 0, -np.inf))), "pose entry not finite")
    c = seg.kf1.camera2
    _refused(lib, with_kf(seg, "kf1", camera2=rep(c, params=poked(c.params, 6, np.nan))), "camera2 parameter not finite")
    _refused(lib, with_kf(seg, "kf2", camera=rep(seg.kf2.camera, precision=float("nan"))), "camera parameter not finite")
    _refused(lib, with_kf(st, "kf1", mbf=float("inf")), "one is not finite")
    _refused(lib, rep(seg, pt1=poked(seg.pt1, (3, 1), np.nan)), "coordinate not finite")
    _refused(lib, rep(seg, pt2=poked(seg.pt2, (19, 0), np.inf)), "coordinate not finite")
    _refused(lib, rep(st, u_right2=poked(st.u_right2, 4, np.nan)), "mvuRight or mvDepth")
    _refused(lib, rep(st, depth1=poked(st.depth1, 0, np.inf)), "mvuRight or mvDepth")
    _refused(lib, with_kf(seg, "kf1", level_sigma2=poked(seg.kf1.level_sigma2, 2, np.nan)), "level table entry not finite")
    _refused(lib, with_kf(seg, "kf2", scale_factors=poked(seg.kf2.scale_factors, 7, np.inf)), "level table entry not finite")
    _refused(lib, rep(seg, ratio_factor=float("nan")), "ratio_factor")
    _refused(lib, rep(seg, th_far_points=float("inf")), "th_far_points")
    # fx / fy equal to 0
    _refused(lib, with_kf(st, "kf1", fx=0.0), "fx or fy is 0")
    _refused(lib, with_kf(st, "kf2", fy=0.0), "fx or fy is 0")
    _refused(lib, with_kf(seg, "kf2", camera=rep(seg.kf2.camera, params=poked(seg.kf2.camera.params, 1, 0.0))), "camera fx or fy is 0")
    _refused(lib, with_kf(seg, "kf1", camera2=rep(c, params=poked(c.params, 0, 0.0))), "camera2 fx or fy is 0")
    _refused(lib, with_kf(seg, "kf1", camera=rep(seg.kf1.camera, type=2)), "neither pinhole nor KannalaBrandt8")
    # an octave outside the level tables, an index outside the keyframe's arrays
    _refused(lib, rep(seg, octave1=poked(seg.octave1, 5, 8)), "octave 8 outside [0, 8) of kf1")
    _refused(lib, rep(seg, octave2=poked(seg.octave2, 6, -1)), "octave -1 outside [0, 8) of kf2")
    _refused(lib, rep(seg, idx1=poked(seg.idx1, 7, seg.kf1.n_keys)), "outside [0, 1000) of kf1")
    _refused(lib, rep(seg, idx2=poked(seg.idx2, 8, -1)), "index -1 outside")
    _refused(lib, with_kf(seg, "kf1", level_sigma2=np.ones(17, F), scale_factors=np.ones(17, F)), "n_levels 17")
    # NULL arrays with a non-zero count
    for field, typ in (("idx2", capi.c_int32_p), ("pt1", capi.c_float_p), ("depth2", capi.c_float_p), ("octave1", capi.c_int32_p)):
        cs, cr, _keep, _ = orb.newpoint_args([seg])
        setattr(cs[0], field, C.cast(None, typ))
        assert lib.osh_orb_triangulate_new_points(None, 1, cs, cr) == capi.OSH_ERR_INVALID and "NULL match array" in capi.last_error(lib)
    cs, cr, _keep, _ = orb.newpoint_args([seg])
    cs[0].kf2.scale_factors = C.cast(None, capi.c_float_p)
    assert lib.osh_orb_triangulate_new_points(None, 1, cs, cr) == capi.OSH_ERR_INVALID and "NULL level table" in capi.last_error(lib)
    assert _call(lib, [seg], results=False) == capi.OSH_ERR_INVALID and "bad arguments" in capi.last_error(lib)
    assert lib.osh_orb_triangulate_new_points(None, -1, None, None) == capi.OSH_ERR_INVALID
    cs, cr, _keep, _ = orb.newpoint_args([seg])
    cs[0].n_matches = -3
    assert lib.osh_orb_triangulate_new_points(None, 1, cs, cr) == capi.OSH_ERR_INVALID and "negative match count" in capi.last_error(lib)
    # sizes beyond the stated limits: the count alone decides, before any array is read
    cs, cr, _keep, _ = orb.newpoint_args([seg])
    assert lib.osh_orb_triangulate_new_points(None, capi.OSH_NEWPOINT_MAX_SEGMENTS + 1, cs, cr) == capi.OSH_ERR_UNSUPPORTED
    assert "segments" in capi.last_error(lib)
    cs, cr, _keep, _ = orb.newpoint_args([seg])
    cs[0].n_matches = capi.OSH_NEWPOINT_MAX_MATCHES + 1
    assert lib.osh_orb_triangulate_new_points(None, 1, cs, cr) == capi.OSH_ERR_UNSUPPORTED and "matches in one call" in capi.last_error(lib)
    # well-formed calls get as far as the missing context; nothing to do needs none either
    assert _call(lib, [seg]) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
    assert _call(lib, [seg.head(0), st.head(0)]) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
    assert _call(lib, []) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)


def test_kernel_library_exports_the_new_entry_and_no_cpp_symbols():
    out = subprocess.run(["nm", "-DC", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "osh_orb_triangulate_new_points" in out and "osh_orb_newpoint_get_times" in out
    assert "ORB_SLAM3::" not in out and "osh::" not in out
    host = subprocess.run(["nm", "-DC", str(capi.HOST_LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "osh_host_newpoint_triangulate_cpu" in host
