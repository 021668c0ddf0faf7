"""osh_orb_sim3_ransac does not depend on what its context ran before: the same bits on fresh contexts and on a long-lived one that
runs large, small and large calls with an MLPnP solve, a two-view reconstruction and a stereo match in between."""
import numpy as np
import pytest

import sim3_ransac_cases as sc
from orb_slam3_study_kr_amd import orb
from orb_slam3_study_kr_amd import synth_mlpnp as sm
from orb_slam3_study_kr_amd import synth_stereo as sst
from orb_slam3_study_kr_amd import synth_two_view as st

pytestmark = pytest.mark.gpu


def assert_same_list(got, ref, what):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        for name in a:
            assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{what}: problem {k}: {name}"


def test_result_does_not_depend_on_what_the_context_ran_before(hip_lib, monkeypatch):
    monkeypatch.setenv("OSH_ZERO_NEW_BUFFERS", "1")
    small = [sc.grid_problem(65, 3, "pinhole-kb8", False)]
    big = [sc.grid_problem(300, 300, "pinhole-pinhole", False), sc.grid_problem(300, 300, "kb8-kb8", True), sc.end_to_end(1, False)]
    mlpnp = [sm.make_problem(seed=21, n=65, iterations=5, min_inliers=6, outlier_share=0.3)]
    two_view = [st.problem(st.make_scene(**st.CASES["general"]), 3)]
    rect = [sst.make_stereo_frame(301, n_left=65, n_right=257, n_levels=3)]
    with orb.OrbMatcher(0) as fresh:
        ref_small = fresh.sim3_ransac(small, debug=True)
    with orb.OrbMatcher(0) as fresh:
        ref_big = fresh.sim3_ransac(big, debug=True)
    with orb.OrbMatcher(0) as fresh:
        ref_score = fresh.sim3_ransac_check_inliers(small[0], sc.transforms(small[0], 1))
    with orb.OrbMatcher(0) as live:
        live.two_view_reconstruct(two_view)
        live.stereo_match(rect)
        assert_same_list(live.sim3_ransac(big, debug=True, fill=0xEE), ref_big, "big after two-view and stereo")
        live.mlpnp_solve(mlpnp)
        assert_same_list(live.sim3_ransac(small, debug=True, fill=0xEE), ref_small, "small after big")
        got = live.sim3_ransac_check_inliers(small[0], sc.transforms(small[0], 1))
        assert np.array_equal(got[0], ref_score[0]) and np.array_equal(got[1], ref_score[1])
        live.stereo_match(rect)
        live.two_view_reconstruct(two_view)
        assert_same_list(live.sim3_ransac(big, debug=True, fill=0xEE), ref_big, "big after small")
        assert_same_list(live.sim3_ransac(small, debug=True, fill=0xEE), ref_small, "small again")
