"""osh_orb_mlpnp_solve does not depend on what its context ran before: the same bits on a fresh context and on one that ran a
two-view reconstruction, a stereo match and larger and smaller MLPnP calls first."""
import numpy as np
import pytest

from orb_slam3_study_kr_amd import orb
from orb_slam3_study_kr_amd import synth_mlpnp as sm
from orb_slam3_study_kr_amd import synth_stereo as ss
from orb_slam3_study_kr_amd import synth_two_view as st

pytestmark = pytest.mark.gpu


def assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k}"


def test_result_does_not_depend_on_what_the_context_ran_before(hip_lib, monkeypatch):
    monkeypatch.setenv("OSH_ZERO_NEW_BUFFERS", "1")
    small = [sm.make_problem(seed=21, n=65, iterations=5, min_inliers=6, outlier_share=0.3)]
    big = [sm.make_problem(seed=22, n=300, iterations=300), sm.make_problem(seed=23, n=130, iterations=40, camera_type=sm.KB8)]
    two_view = [st.problem(st.make_scene(**st.CASES["general"]), 3)]
    rect = [ss.make_stereo_frame(301, n_left=65, n_right=257, n_levels=3)]
    with orb.OrbMatcher(0) as fresh:
        ref_small = fresh.mlpnp_solve(small, debug=True)
    with orb.OrbMatcher(0) as fresh:
        ref_big = fresh.mlpnp_solve(big, debug=True)
    with orb.OrbMatcher(0) as live:
        live.two_view_reconstruct(two_view)
        live.stereo_match(rect)
        assert_same_list(live.mlpnp_solve(small, debug=True, fill=0xEE), ref_small, "small after two-view and stereo")
        assert_same_list(live.mlpnp_solve(big, debug=True, fill=0xEE), ref_big, "big after small")
        live.stereo_match(rect)
        live.two_view_reconstruct(two_view)
        assert_same_list(live.mlpnp_solve(small, debug=True, fill=0xEE), ref_small, "small after big")


def assert_same_list(got, ref, what):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert_same(a, b, f"{what}: problem {k}")
