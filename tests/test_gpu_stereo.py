"""osh_orb_stereo_match and Frame::ComputeStereoMatches on the device against the numpy restatement of reference
src/Frame.cc:816-986 (tests/stereo_numpy.py): float32 outputs as bit patterns, every stage output as integers, for every
keypoint, without tolerance."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import stereo_numpy as sn
from orb_slam3_study_kr_amd import capi, orb, synth
from orb_slam3_study_kr_amd import synth_stereo as ss

pytestmark = pytest.mark.gpu
F = np.float32


def _check(m, frames, what, borders=None):
    got = m.stereo_match(frames, stages=True, borders=borders)
    for k, fr in enumerate(frames):
        sn.assert_same(got[k], sn.compute_stereo_matches(fr), what=f"{what}[{k}]")
    return got


@pytest.mark.parametrize("name", [n for n, _ in sn.CASES])
def test_committed_cases_equal_the_restatement(hip_lib, name):
    fr = ss.make_stereo_frame(**dict(sn.CASES)[name])
    with orb.OrbMatcher(0) as m:
        _check(m, [fr], name)


def test_known_answer_frames(hip_lib):
    frames = [ss.make_shift_frame(3, 5)[0], ss.make_shift_frame(4, 0)[0], ss.make_shift_frame(5, 2, constant=True)[0]]
    with orb.OrbMatcher(0) as m:
        got = _check(m, frames, "shift")
    assert (got[2]["stage"] == capi.OSH_STEREO_BORDER_INC).all()      # a frame with no accepted keypoint: no median


@pytest.mark.parametrize("n_levels", range(1, 9))
def test_one_to_eight_pyramid_levels(hip_lib, n_levels):
    fr = ss.make_stereo_frame(40 + n_levels, n_left=600, n_levels=n_levels)
    with orb.OrbMatcher(0) as m:
        _check(m, [fr], f"levels={n_levels}", borders=[n_levels])


@pytest.mark.parametrize("n_left,n_right", [(0, 0), (0, 700), (1, 1), (5, 0), (63, 65), (64, 256), (65, 257), (700, 3), (1000, 4000),
                                            (4000, 1000), (4000, 4000)])
def test_keypoint_counts(hip_lib, n_left, n_right):
    fr = ss.make_stereo_frame(100 + n_left + n_right, n_left=n_left, n_right=n_right)
    assert fr.left_xy.shape[0] == n_left and fr.right_xy.shape[0] == n_right
    with orb.OrbMatcher(0) as m:
        _check(m, [fr], f"{n_left}x{n_right}")


def test_frames_without_accepted_keypoints(hip_lib):
    frames = [ss.make_stereo_frame(61, n_left=300, constant=True), ss.make_stereo_frame(62, n_left=200, n_right=0),
              ss.make_stereo_frame(63, n_left=300, bf=0.001)]       # bf / b below every disparity
    with orb.OrbMatcher(0) as m:
        got = _check(m, frames, "none accepted")
    for g in got:
        assert (g["u_right"] == -1).all() and (g["depth"] == -1).all()


def _mixed_batch():
    return [ss.make_stereo_frame(71, n_left=1500), ss.make_stereo_frame(72, n_left=40, extra_right=0.0),
            ss.make_stereo_frame(73, n_left=0), ss.make_stereo_frame(74, n_left=900, n_levels=3, median_band=True),
            ss.make_stereo_frame(75, n_left=300, width=400, height=300, n_levels=5, zero_band=True),
            ss.make_shift_frame(76, 6)[0], ss.make_stereo_frame(77, n_left=2500, edge_guard=True)]


def test_batch_equals_single_calls(hip_lib):
    frames = _mixed_batch()
    borders = [0, 3, 0, 19, 1, 0, 7]
    with orb.OrbMatcher(0) as m:
        batch = _check(m, frames, "batch", borders=borders)
        for k, fr in enumerate(frames):
            one = m.stereo_match([fr], stages=True)[0]
            sn.assert_same(one, batch[k], what=f"single {k}")


@pytest.fixture()
def zero_new_buffers():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OSH_ZERO_NEW_BUFFERS", "1")
        yield


def test_long_lived_context_equals_fresh_contexts(hip_lib, zero_new_buffers):
    """A matcher that ran other osh_orb_* calls and larger frames first returns, for every later stereo call, bit for bit what a
    fresh matcher returns."""
    big = [ss.make_stereo_frame(81, n_left=4000), ss.make_stereo_frame(82, n_left=3000, median_band=True)]
    later = [[ss.make_stereo_frame(83, n_left=700, n_levels=4)], [ss.make_stereo_frame(84, n_left=30, extra_right=0.0)],
             _mixed_batch()[3:6], [ss.make_stereo_frame(85, n_left=1500, low_contrast=True)]]
    pair = synth.make_orb_pair(9, 2000, 2000)
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, (300, 32), dtype=np.uint8), rng.integers(0, 256, (200, 32), dtype=np.uint8)
    with orb.OrbMatcher(0) as m:
        m.search([pair])
        m.stereo_match(big, stages=True)
        m.distance_matrix(a, b)
        for k, frames in enumerate(later):
            got = m.stereo_match(frames, stages=True)
            m.search([pair], windowed=False)
            with orb.OrbMatcher(0) as fresh:
                ref = fresh.stereo_match(frames, stages=True)
            for j in range(len(frames)):
                sn.assert_same(got[j], ref[j], what=f"step {k} frame {j}")
                sn.assert_same(got[j], sn.compute_stereo_matches(frames[j]), what=f"step {k} frame {j} restatement")


def _host_compute(fr, border):
    lib = capi.load_host_library()
    h, keep = sn.host_input(fr)
    u, d = np.zeros(h.n_left, F), np.zeros(h.n_left, F)
    rc = lib.osh_host_compute_stereo_matches(C.byref(h), border, capi.ptr(u, capi.c_float_p), capi.ptr(d, capi.c_float_p))
    assert rc == 0, rc
    return dict(u_right=u, depth=d)


@pytest.mark.parametrize("border", [0, 19])
def test_frame_compute_stereo_matches_equals_the_restatement(hip_lib, border):
    """Through the mangled Frame::ComputeStereoMatches of the host layer, pyramid levels stored as views into bordered images."""
    for name in ("seed1", "median_band", "zero_band", "edge_guard"):
        fr = ss.make_stereo_frame(**dict(sn.CASES)[name])
        exp = sn.compute_stereo_matches(fr)
        sn.assert_same(_host_compute(fr, border), exp, keys=("u_right", "depth"), what=f"{name} border {border}")
        assert (exp["u_right"] >= 0).sum() > 100
    empty = ss.make_stereo_frame(91, n_left=0)
    assert _host_compute(empty, border)["u_right"].shape == (0,)


def _undefined_frame():
    """Inputs on which the reference's behaviour is undefined: right keypoints whose rows leave the image, left keypoints whose
    row is outside, keypoints so close to a border that a patch leaves its level."""
    fr = ss.make_stereo_frame(95, n_left=400, n_levels=3)
    lxy, rxy = fr.left_xy.copy(), fr.right_xy.copy()
    h, w = fr.left_pyramid[0].shape
    p = fr.partner
    have = np.nonzero(p >= 0)[0]
    a, b, c, d = have[:20], have[20:40], have[40:60], have[60:80]
    lxy[a, 1] = 2.0; rxy[p[a], 1] = 1.0                     # patch rows above the image; right rows -2 .. 4 partly outside
    lxy[b, 1] = h - 2.0; rxy[p[b], 1] = h - 1.5             # patch rows below; right rows beyond the last one
    lxy[c, 1] = h + 4.0; rxy[p[c], 1] = h + 4.0             # left row outside the row table
    lxy[d, 0] = 3.0 * fr.scale_factors[fr.left_octave[d]]; rxy[p[d], 0] = lxy[d, 0] - 1.0   # left patch leaves on the left, right strip too
    lxy[have[80:90], 1] = -3.0
    return dataclasses.replace(fr, left_xy=lxy, right_xy=rxy)


def test_undefined_inputs_are_defined_skips(hip_lib):
    fr = _undefined_frame()
    exp = sn.compute_stereo_matches(fr)
    assert exp["undefined"][0] > 0 and exp["undefined"][1] > 0 and exp["undefined"][2] > 0
    assert (exp["stage"] == capi.OSH_STEREO_PATCH).sum() >= 10 and (exp["stage"] == capi.OSH_STEREO_ACCEPTED).sum() >= 50
    with orb.OrbMatcher(0) as m:
        got = m.stereo_match([fr], stages=True, borders=[2])[0]
    sn.assert_same(got, exp, what="undefined inputs")
    sn.assert_same(_host_compute(fr, 2), exp, keys=("u_right", "depth"), what="undefined inputs, Frame")


def test_malformed_input_is_refused(hip_lib):
    fr = ss.make_stereo_frame(97, n_left=100, n_levels=3)
    used = int(fr.left_octave[0])
    with orb.OrbMatcher(0) as m:
        missing = dataclasses.replace(fr, right_pyramid=[None if l == used else p for l, p in enumerate(fr.right_pyramid)])
        with pytest.raises(capi.OshError) as e:
            m.stereo_match([missing])
        assert e.value.code == capi.OSH_ERR_INVALID and "NULL" in str(e.value)
        sf, isf = ss.scale_pyramid(capi.OSH_STEREO_MAX_LEVELS + 1)
        too_many = dataclasses.replace(fr, scale_factors=sf, inv_scale_factors=isf,
                                       left_pyramid=fr.left_pyramid + [fr.left_pyramid[-1]] * (capi.OSH_STEREO_MAX_LEVELS - 2),
                                       right_pyramid=fr.right_pyramid + [fr.right_pyramid[-1]] * (capi.OSH_STEREO_MAX_LEVELS - 2))
        with pytest.raises(capi.OshError) as e:
            m.stereo_match([too_many])
        assert e.value.code == capi.OSH_ERR_INVALID
        bad_oct = dataclasses.replace(fr, left_octave=np.where(np.arange(100) == 5, 3, fr.left_octave).astype(np.int32))
        with pytest.raises(capi.OshError):
            m.stereo_match([bad_oct])
        nan = fr.left_xy.copy(); nan[7, 0] = np.nan
        with pytest.raises(capi.OshError):
            m.stereo_match([dataclasses.replace(fr, left_xy=nan)])
        _check(m, [fr], "after refusals")
        # a level no left keypoint names may be NULL
        few = ss.make_stereo_frame(98, n_left=30, n_levels=8)
        unused = [l for l in range(1, 8) if l not in set(few.left_octave.tolist())]
        assert unused
        ok = dataclasses.replace(few, left_pyramid=[None if l in unused else p for l, p in enumerate(few.left_pyramid)],
                                 right_pyramid=[None if l in unused else p for l, p in enumerate(few.right_pyramid)])
        sn.assert_same(m.stereo_match([ok], stages=True)[0], sn.compute_stereo_matches(few), what="unused level NULL")


def test_kernel_library_exports_no_cpp_symbols(hip_lib):
    import subprocess
    out = subprocess.run(["nm", "-DC", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "ORB_SLAM3::" not in out
    assert "osh_orb_stereo_match" in out
