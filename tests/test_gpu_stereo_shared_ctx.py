"""osh_orb_stereo_match, osh_orb_fisheye_stereo_match and osh_kb8_triangulate in turn on one osh_orb_ctx: they share the context's
attachment slots and the keypoint-batch staging of csrc/orb_stage.h, and every call returns, bit for bit, what the same call
returns on a context of its own.  The shapes sit on the edges of the shared code: a frame with an empty left side next to a full one
(bases, the scatter of nothing), counts one past a wavefront and one past an LDS tile, and a right set shorter than one tile."""
import numpy as np
import pytest

from orb_slam3_study_kr_amd import orb
from orb_slam3_study_kr_amd import synth_fisheye as sf
from orb_slam3_study_kr_amd import synth_stereo as ss

pytestmark = pytest.mark.gpu


@pytest.fixture()
def zero_new_buffers():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OSH_ZERO_NEW_BUFFERS", "1")
        yield


def _assert_same_bits(got, ref, what):
    """Every array of two results (a dict, or a list of per-frame dicts) equal: floats as bit patterns."""
    got, ref = (got, ref) if isinstance(got, list) else ([got], [ref])
    assert len(got) == len(ref), what
    for k, (g, r) in enumerate(zip(got, ref)):
        assert set(g) == set(r) and len(g) >= 3, (what, k)
        for name in g:
            a, b = g[name], r[name]
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k, name)
            if a.dtype == np.float32:
                a, b = a.view(np.uint32), b.view(np.uint32)
            assert np.array_equal(a, b), f"{what}[{k}]: {name}"


def test_stereo_entries_share_one_context(hip_lib, zero_new_buffers):
    rect = [ss.make_stereo_frame(301, n_left=65, n_right=257, n_levels=3), ss.make_stereo_frame(302, n_left=0, n_right=40, n_levels=3)]
    shrunk = [ss.make_stereo_frame(303, n_left=700, n_right=3, n_levels=3)]
    fish = [sf.make_fisheye_frame(304, n_left=64, n_right=256, mono_left=10, mono_right=20),
            sf.make_fisheye_frame(305, n_left=1, n_right=2, mono_left=0, mono_right=0)]
    assert [(f.left_xy.shape[0], f.right_xy.shape[0]) for f in rect + shrunk + fish] == [(65, 257), (0, 40), (700, 3), (64, 256), (1, 2)]
    assert (fish[0].mono_left, fish[0].mono_right) == (10, 20)
    fr = fish[0]
    rig = orb.kb8_rig(fr.cam1, fr.cam2, fr.precision1, fr.precision2, fr.Rlr, fr.tlr)
    pairs = (fr.right_xy[:65], fr.right_xy[65:130], fr.level_sigma2[fr.right_octave[:65]], fr.level_sigma2[fr.right_octave[65:130]])
    steps = [("stereo", lambda m: m.stereo_match(rect, stages=True)),
             ("fisheye", lambda m: m.fisheye_stereo_match(fish, stages=True)),
             ("triangulate", lambda m: m.kb8_triangulate(rig, *pairs)),
             ("stereo, smaller", lambda m: m.stereo_match(shrunk, stages=True)),
             ("fisheye again", lambda m: m.fisheye_stereo_match(fish, stages=True))]
    with orb.OrbMatcher(0) as shared:
        for what, call in steps:
            got = call(shared)
            with orb.OrbMatcher(0) as fresh:
                ref = call(fresh)
            _assert_same_bits(got, ref, what)
    assert got[0]["left_to_right"].shape == (64,) and got[1]["right_to_left"].shape == (2,)


def test_times_before_any_stereo_call_are_zero(hip_lib):
    with orb.OrbMatcher(0) as m:
        assert np.array_equal(m.stereo_times(), np.zeros(4)) and np.array_equal(m.fisheye_stereo_times(), np.zeros(4))
