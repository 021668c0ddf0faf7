"""The pose side of the first round of optimize() (Hpp, b_p and through them computeLambdaInit) runs in an instantiation of
k_schur_fused that holds nothing of the Schur side (csrc/lba_schur_items.h: POSE_ONLY); OSH_LBA_POSE_PASS_FULL, read once per upload,
keeps the full kernel called with mode 0 for that launch.  The two must give the same bits: the lambda of the first iteration, which
is the first number that depends on Hpp, and the whole result of optimize().
The windows: the four of tests/test_gpu_schur_long_items.py (3, 5, 8 and 12 optimisable keyframes: the 16 x 4, 12 x 5 and 8 x 8 lane
mappings, partial last chunks, symmetric items next to cross items), cut at 256 landmarks per item as there; a window of 2 keyframes
and 300 points; the fisheye-rig window of tests/golden/lba_tiny_rig.npz (the KannalaBrandt8 instantiation).  Each alone, and all in one
call."""
import numpy as np
import pytest

from helpers import load_lba_fixture
from orb_slam3_study_kr_amd import lba, synth
from test_gpu_schur_long_items import SPECS

pytestmark = pytest.mark.gpu

FIELDS = ("chi2_trace", "lambda_trace", "trials_trace", "pose_qt", "points", "edge_chi2", "edge_depth_pos")


def _windows():
    ws = {}
    for n in sorted(SPECS):
        sp = dict(SPECS[n])
        ws[f"kf{n}"] = synth.make_window(sp.pop("seed"), stereo=True, **sp)
    ws["kf2"] = synth.make_window(9311, n_free=2, n_fixed=1, n_points=300, stereo=True, track_len=(2, 3))
    ws["rig"] = load_lba_fixture("lba_tiny_rig")[0]
    return ws


@pytest.fixture(scope="module")
def runs(hip_lib):
    """mode -> case -> results; case: a window's name (uploaded alone) or "together" (all of them in one call)"""
    ws = _windows()
    cases = {name: [w] for name, w in ws.items()}
    cases["together"] = list(ws.values())
    out = {}
    mp = pytest.MonkeyPatch()
    mp.setenv("OSH_LBA_ITEM_MAX", "256")
    try:
        with lba.LbaSolver(0) as s:
            for mode in ("pose_only", "full"):
                if mode == "full":
                    mp.setenv("OSH_LBA_POSE_PASS_FULL", "1")
                else:
                    mp.delenv("OSH_LBA_POSE_PASS_FULL", raising=False)
                out[mode] = {case: s.solve(batch) for case, batch in cases.items()}
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("case", ["kf3", "kf5", "kf8", "kf12", "kf2", "rig", "together"])
def test_pose_only_pass_gives_the_bits_of_the_full_kernel(runs, case):
    got, ctl = runs["pose_only"][case], runs["full"][case]
    assert len(got) == len(ctl) == (6 if case == "together" else 1)
    for g, c in zip(got, ctl):
        assert g.iterations > 0 and (g.iterations, g.trials) == (c.iterations, c.trials)
        assert g.lambda_trace[0] == c.lambda_trace[0] and g.lambda_trace[0] > 0
        assert g.chi2_initial == c.chi2_initial
        for name in FIELDS:
            np.testing.assert_array_equal(getattr(g, name), getattr(c, name), err_msg=name)
