"""The windows of the solver tests (test_solve_reference_cpu.py chooses and vets them on the CPU, test_gpu_solve.py runs them).

Stereo windows with few landmarks (about 40 per keyframe: a case costs milliseconds on the device) in two track styles per size:
    short   tracks of 2 to 4 keyframes: a ragged column envelope with empty blocks above it
    long    tracks longer than the window, the keyframes close enough to share their landmarks: a dense S
The sizes are the edges of the two factorisations (see the tables in test_gpu_solve.py)."""
import numpy as np

from orb_slam3_study_kr_amd import synth

LAMBDAS = (1e-3, 1e-8)
STYLES = ("short", "long")
LDS_POSES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 40, 41)
BIG_POSES = (1, 5, 6, 11, 16, 17, 32, 33, 43, 100)
SMALL_SPECS = sorted({(p, s) for p in LDS_POSES + BIG_POSES for s in STYLES})
# the natural switch points of the selection rule (csrc/solve_plan.h), no override: (poses, landmarks)
SWITCH_LDS = ((116, 2500), (235, 3000))
SWITCH_BIG = ((437, 6000), (438, 6000), (439, 6000))
# the first size (with two fixed keyframes) at which x_p and the poses no longer fit k_backsub's LDS beside the trial poses
BACKSUB_GLOBAL = ((394, 5000),)

_CACHE = {}


def window(poses, style, n_points=None):
    key = (poses, style, n_points)
    if key not in _CACHE:
        K = poses + 2
        kw = dict(track_len=(2, 4)) if style == "short" else dict(track_len=(K, K), kf_spacing=min(0.25, 8.0 / K))
        # (the yaw of the default drift reaches a radian at the ends of a 440-keyframe window: its last cameras look past the
        #  landmarks, and a keyframe with two edges leaves S singular up to lambda)
        _CACHE[key] = synth.make_window(7000 + 10 * poses + STYLES.index(style), n_free=poses, n_fixed=2,
                                        n_points=n_points or max(80, 40 * poses), stereo=True, yaw_drift=min(0.02, 1.0 / K), **kw)
    return _CACHE[key]


def switch_window(poses, n_points):
    return window(poses, "short", n_points)


ZERO_PIVOT_POSE = 7     # unknowns 42 .. 47: the second panel of big_solve.h and of NB = 24, the fourth of NB = 12, the eighth of NB = 6


def zero_pivot_window():
    """Nine optimisable poses, long tracks, and pose 7 stripped of all its edges: its block row and column of S are zero up to
    lambda, so a trial at lambda = 0 meets an exactly-zero pivot at unknown 42.  Every landmark keeps its other observers."""
    import dataclasses
    w = window(9, "long")
    keep = w.edge_pose != ZERO_PIVOT_POSE
    w = dataclasses.replace(w, **{name: np.ascontiguousarray(getattr(w, name)[keep])
                                  for name in ("edge_pose", "edge_point", "edge_kind", "edge_obs", "edge_info")})
    assert np.bincount(w.edge_point, minlength=w.n_points).min() >= 2
    return w


def edgeless_landmark_window():
    """The window of test_gpu_lba.py::test_stop_flag_zero_iterations_and_empty_cases that its comment calls a zero-pivot window: a
    landmark seen by fixed keyframes only.  (Every pose keeps edges and lambda is positive: no pivot of it is zero, see
    test_solve_reference_cpu.py.)"""
    w2 = synth.make_window(6, n_free=3, n_fixed=2, n_points=40, track_len=(2, 5))
    fixed_seen = np.unique(w2.edge_point[w2.edge_pose >= w2.n_free])
    j = int(fixed_seen[0])
    keep = ~((w2.edge_point == j) & (w2.edge_pose < w2.n_free))
    for name in ("edge_pose", "edge_point", "edge_kind", "edge_obs", "edge_info"):
        setattr(w2, name, np.ascontiguousarray(getattr(w2, name)[keep]))
    return w2
