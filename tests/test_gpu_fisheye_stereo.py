"""osh_orb_fisheye_stereo_match, osh_kb8_triangulate and Frame::ComputeStereoFishEyeMatches on the device against the numpy
restatement of reference src/Frame.cc:1131-1171 and KannalaBrandt8::TriangulateMatches (tests/fisheye_stereo_numpy.py): the
neighbours, the ratio decision and cosParallaxRays bit for bit for every keypoint; depth and the 3D point equal or adjacent in
float32 (both sides take the singular vector in float64 from the same float32 matrix, so only a rounding boundary can part them);
stage and both match arrays equal for every match the restatement does not mark borderline."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import fisheye_stereo_numpy as fn
from orb_slam3_study_kr_amd import capi, orb, synth
from orb_slam3_study_kr_amd import synth_fisheye as sf
from orb_slam3_study_kr_amd import synth_stereo as ss

pytestmark = pytest.mark.gpu
F = np.float32
KNOWN_PAIRS, PLAIN, PLAIN_RIG = fn.KNOWN_PAIRS, fn.PLAIN, fn.PLAIN_RIG


@functools.lru_cache(maxsize=None)
def made(**kw):
    """A generated frame and its restatement, computed once per argument set."""
    fr = sf.make_fisheye_frame(**kw)
    return fr, fn.compute(fr)


def _check(m, specs, what):
    frames = [made(**kw)[0] for kw in specs]
    got = m.fisheye_stereo_match(frames, stages=True)
    for k, kw in enumerate(specs):
        fn.assert_matches(got[k], made(**kw)[1], what=f"{what}[{k}]")
    return frames, got


@pytest.mark.parametrize("name", [n for n, _ in fn.CASES])
def test_committed_cases_equal_the_restatement(hip_lib, name):
    with orb.OrbMatcher(0) as m:
        _, got = _check(m, [dict(fn.CASES)[name]], name)
    if name == "no_pair":
        assert (got[0]["stage"] <= capi.OSH_FSTEREO_NO_PAIR).all() and (got[0]["left_to_right"] == -1).all()


@pytest.mark.parametrize("n_left,n_right", [(0, 0), (0, 40), (1, 1), (1, 2), (2, 1), (63, 65), (64, 256), (65, 257), (700, 3), (1500, 1500)])
def test_keypoint_counts(hip_lib, n_left, n_right):
    kw = dict(seed=100 + n_left + n_right, n_left=n_left, n_right=n_right, mono_left=0, mono_right=0)
    fr = made(**kw)[0]
    assert fr.left_xy.shape[0] == n_left and fr.right_xy.shape[0] == n_right
    with orb.OrbMatcher(0) as m:
        _check(m, [kw], f"{n_left}x{n_right}")


@pytest.mark.parametrize("mono_left,mono_right", [(0, 20), (300, 20), (10, 299), (10, 298)])
def test_mono_settings(hip_lib, mono_left, mono_right):
    """mono_left = 0; mono_left = n_left (nothing to match); one train row (every query is "no pair"); two train rows."""
    kw = dict(seed=7, n_left=300, n_right=300, mono_left=mono_left, mono_right=mono_right)
    with orb.OrbMatcher(0) as m:
        _, got = _check(m, [kw], f"mono {mono_left}/{mono_right}")
    stage = got[0]["stage"]
    if mono_left == 300:
        assert (stage == capi.OSH_FSTEREO_OUTSIDE).all()
    if mono_right == 299:
        assert (stage[mono_left:] == capi.OSH_FSTEREO_NO_PAIR).all()
    if mono_right == 298:
        assert (stage[mono_left:] >= capi.OSH_FSTEREO_RATIO).all() and set(got[0]["best_right"][mono_left:]) <= {298, 299}


def test_full_depth_range(hip_lib):
    """Points spread over 0.3 m to 50 m, where the parallax test rejects most of them: the committed cases keep such points few
    because the restatement calls every cosine from 0.9988 up borderline; here cosParallaxRays and with it the parallax decision are
    still compared bit for bit for every one of them."""
    kw = dict(seed=41, n_left=900, n_right=900, n_far=350)
    e = made(**kw)[1]
    assert (e["stage"] == capi.OSH_FSTEREO_PARALLAX).sum() >= 150
    with orb.OrbMatcher(0) as m:
        got = _check(m, [kw], "full depth range")[1][0]
    assert np.array_equal(got["stage"] == capi.OSH_FSTEREO_PARALLAX, e["stage"] == capi.OSH_FSTEREO_PARALLAX)


MIXED = (dict(seed=21, n_left=900, n_right=700), dict(seed=22, n_left=40, n_right=300, mono_left=0, mono_right=0, tz=-0.03),
         dict(seed=23, n_left=0, n_right=10), dict(seed=24, n_left=500, n_right=520, tz=-0.03, mono_left=100, mono_right=3),
         dict(seed=25, n_left=65, n_right=1, mono_left=0, mono_right=0), dict(seed=26, n_left=300, n_right=300, shared=0.3),
         dict(seed=27, n_left=1100, n_right=1300, mono_left=64, mono_right=256))


def test_batch_equals_single_calls(hip_lib):
    with orb.OrbMatcher(0) as m:
        frames, batch = _check(m, MIXED, "batch")
        for k, fr in enumerate(frames):
            fn.assert_same(m.fisheye_stereo_match([fr], stages=True)[0], batch[k], what=f"single {k}")


@pytest.fixture()
def zero_new_buffers():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OSH_ZERO_NEW_BUFFERS", "1")
        yield


def test_long_lived_context_equals_fresh_contexts(hip_lib, zero_new_buffers):
    """A matcher that ran search, stereo_match, distance_matrix and a larger fisheye frame first returns, for every later fisheye
    call, bit for bit what a fresh matcher returns."""
    later = [[MIXED[3]], [MIXED[1]], list(MIXED[4:7]), [dict(fn.CASES)["behind"]]]
    pair = synth.make_orb_pair(9, 2000, 2000)
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, (300, 32), dtype=np.uint8), rng.integers(0, 256, (200, 32), dtype=np.uint8)
    with orb.OrbMatcher(0) as m:
        m.search([pair])
        m.stereo_match([ss.make_stereo_frame(81, n_left=3000)], stages=True)
        m.distance_matrix(a, b)
        m.fisheye_stereo_match([made(seed=31, n_left=2500, n_right=2500)[0]], stages=True)
        for k, specs in enumerate(later):
            frames, got = _check(m, specs, f"step {k}")
            m.search([pair], windowed=False)
            with orb.OrbMatcher(0) as fresh:
                ref = fresh.fisheye_stereo_match(frames, stages=True)
            for j in range(len(frames)):
                fn.assert_same(got[j], ref[j], what=f"step {k} frame {j}")


def test_triangulation_entry(hip_lib):
    rig = orb.kb8_rig(*PLAIN_RIG)
    names = list(KNOWN_PAIRS)
    with orb.OrbMatcher(0) as m:
        got = m.kb8_triangulate(rig, [KNOWN_PAIRS[n][0] for n in names], [KNOWN_PAIRS[n][1] for n in names], [1.0] * 3, [1.0] * 3)
        for i, n in enumerate(names):
            _, _, ret, X = KNOWN_PAIRS[n]
            if ret is not None:
                assert got["ret"][i] == ret and not got["p3d"][i].any(), n
            else:
                assert got["ret"][i] == got["p3d"][i][2] and np.allclose(got["p3d"][i], X, rtol=1e-5, atol=1e-6), n   # as in the CPU test
        assert got["cos_parallax"][names.index("identical_rays")] == 1.0
        # the hand-made pairs as a frame: the frame call returns the same
        pf = sf.make_pairs_frame([(KNOWN_PAIRS[n][0], KNOWN_PAIRS[n][1]) for n in names], PLAIN, PLAIN, PLAIN_RIG[4], PLAIN_RIG[5])
        fg = m.fisheye_stereo_match([pf], stages=True)[0]
        assert list(fg["stage"]) == [capi.OSH_FSTEREO_ACCEPTED, capi.OSH_FSTEREO_PARALLAX, capi.OSH_FSTEREO_BEHIND_1]
        assert fg["depth"][0] == got["ret"][0] and np.array_equal(fg["p3d"][0], got["p3d"][0])
        # the ratio-accepted pairs of a generated frame
        fr, e = made(**dict(fn.CASES)["ahead"])
        frame = m.fisheye_stereo_match([fr], stages=True)[0]
        idx = np.nonzero(frame["stage"] >= capi.OSH_FSTEREO_PARALLAX)[0]
        r = frame["best_right"][idx]
        sig = fr.level_sigma2
        tri = m.kb8_triangulate(orb.kb8_rig(*fn.rig_of(fr)), fr.left_xy[idx], fr.right_xy[r], sig[fr.left_octave[idx]], sig[fr.right_octave[r]])
    assert np.array_equal(tri["cos_parallax"].view(np.uint32), frame["cos_parallax"][idx].view(np.uint32))
    acc = frame["stage"][idx] == capi.OSH_FSTEREO_ACCEPTED
    assert np.array_equal(tri["ret"] > F(0.0001), acc)
    assert np.array_equal(tri["ret"][acc].view(np.uint32), frame["depth"][idx][acc].view(np.uint32))
    assert np.array_equal(tri["p3d"][acc].view(np.uint32), frame["p3d"][idx][acc].view(np.uint32))
    code = {-1.0: capi.OSH_FSTEREO_PARALLAX, -2.0: capi.OSH_FSTEREO_BEHIND_1, -3.0: capi.OSH_FSTEREO_BEHIND_2,
            -4.0: capi.OSH_FSTEREO_REPROJ_1, -5.0: capi.OSH_FSTEREO_REPROJ_2}
    for i in np.nonzero(tri["ret"] < 0)[0]:
        assert frame["stage"][idx][i] == code[float(tri["ret"][i])]


def _host_compute(fr, pinhole=0):
    lib = capi.load_host_library()
    c = np.ascontiguousarray
    a = dict(lxy=c(fr.left_xy, F), loct=c(fr.left_octave, np.int32), ldesc=c(fr.left_desc, np.uint8), rxy=c(fr.right_xy, F),
             roct=c(fr.right_octave, np.int32), rdesc=c(fr.right_desc, np.uint8), sig=c(fr.level_sigma2, F))
    h = capi.HostFisheyeInput()
    orb.fill_fisheye_frame(h, fr, a)
    nl, nr = h.n_left, h.n_right
    o = dict(left_to_right=np.zeros(nl, np.int32), right_to_left=np.zeros(nr, np.int32), depth=np.zeros(nl, F), p3d=np.zeros((nl, 3), F),
             u_right=np.zeros(nl, F))
    rc = lib.osh_host_compute_fisheye_stereo_matches(C.byref(h), pinhole, capi.ptr(o["left_to_right"], capi.c_int32_p),
                                                     capi.ptr(o["right_to_left"], capi.c_int32_p), capi.ptr(o["depth"], capi.c_float_p),
                                                     capi.ptr(o["p3d"], capi.c_float_p), capi.ptr(o["u_right"], capi.c_float_p))
    assert rc == 0, rc
    return o


def test_frame_compute_stereo_fisheye_matches_equals_the_c_abi(hip_lib, capfd):
    """Through the mangled Frame::ComputeStereoFishEyeMatches of the host layer."""
    with orb.OrbMatcher(0) as m:
        for name in ("ahead", "behind", "shared", "mono"):
            fr, e = made(**dict(fn.CASES)[name])
            exp = m.fisheye_stereo_match([fr])[0]
            got = _host_compute(fr)
            for k in ("left_to_right", "right_to_left"):
                assert np.array_equal(got[k], exp[k]), (name, k)
            for k in ("depth", "p3d"):
                assert np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), (name, k)
            assert (got["u_right"] == -1).all() and (got["left_to_right"] >= 0).sum() > 100
    empty = _host_compute(made(seed=91, n_left=0, n_right=0)[0])
    assert empty["left_to_right"].shape == (0,) and empty["right_to_left"].shape == (0,)
    capfd.readouterr()
    fr = made(**dict(fn.CASES)["ahead"])[0]
    refused = _host_compute(fr, pinhole=1)
    assert (refused["left_to_right"] == -1).all() and (refused["right_to_left"] == -1).all() and (refused["depth"] == -1).all()
    assert "ComputeStereoFishEyeMatches" in capfd.readouterr().err


def test_malformed_input_is_refused(hip_lib):
    kw = dict(seed=11, n_left=50, n_right=40, mono_left=5, mono_right=4)
    fr = made(**kw)[0]
    rep = dataclasses.replace
    xy = fr.left_xy.copy(); xy[3, 0] = np.nan
    cam = fr.cam1.copy(); cam[0] = np.inf
    R = fr.Rlr.copy(); R[1, 1] = np.nan
    bad = [rep(fr, mono_left=51), rep(fr, mono_left=-1), rep(fr, mono_right=41), rep(fr, mono_right=-1),
           rep(fr, left_octave=np.full(50, 8, np.int32)), rep(fr, right_octave=np.full(40, -1, np.int32)), rep(fr, left_xy=xy),
           rep(fr, cam1=cam), rep(fr, Rlr=R), rep(fr, precision2=float("inf"))]
    with orb.OrbMatcher(0) as m:
        for k, b in enumerate(bad):
            with pytest.raises(capi.OshError) as e:
                m.fisheye_stereo_match([fr, b])
            assert e.value.code == capi.OSH_ERR_INVALID, k
        cf, cr, _keep, _ = orb.fisheye_stereo_args([fr])
        cf[0].right_xy = C.cast(None, capi.c_float_p)
        assert m.lib.osh_orb_fisheye_stereo_match(m.ctx, 1, cf, cr) == capi.OSH_ERR_INVALID
        with pytest.raises(capi.OshError):
            m.kb8_triangulate(orb.kb8_rig(PLAIN, PLAIN, 1e-6, 1e-6, np.eye(3), [np.nan, 0, 0]), [[1, 2]], [[3, 4]], [1], [1])
        with pytest.raises(capi.OshError):
            m.kb8_triangulate(orb.kb8_rig(*PLAIN_RIG), [[1, np.inf]], [[3, 4]], [1], [1])
        _check(m, [kw, dict(fn.CASES)["mono"]], "after refusals")
        assert m.kb8_triangulate(orb.kb8_rig(*PLAIN_RIG), [KNOWN_PAIRS["crossed"][0]], [KNOWN_PAIRS["crossed"][1]], [1], [1])["ret"][0] == -2.0
