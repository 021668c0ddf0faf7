"""The computePose cases the MLPnP tests share (tests/test_mlpnp_cpu.py, tests/test_gpu_mlpnp.py): minimal sets drawn from the
inliers only and the refine of the true inlier set, for a Pinhole and a KannalaBrandt8 scene and for a scene on the plane z = 0, each
with its numpy reference (computed once), and the measured spreads the device bound comes from."""
import functools

import numpy as np

import mlpnp_numpy as mn
from orb_slam3_study_kr_amd import synth_mlpnp as sm

N_SETS = 16

# Largest (rotation angle [rad], translation norm) difference between the host build of csrc/mlpnp.h and the numpy restatement over
# pose_cases(), measured on the CPU (tests/test_mlpnp_cpu.py::test_measured_spreads asserts that they still hold), general scenes
# and the z = 0 plane apart; the scale beside them: numpy FP64 against the same Gauss-Newton rerun in np.longdouble.
HOST_VS_NUMPY = {"general": (2.4e-15, 4.5e-15), "planar": (7.7e-12, 8.2e-11)}
NUMPY_VS_LONGDOUBLE = {"general": (3.6e-16, 9.2e-16), "planar": (0.0, 0.0)}   # the planar Gauss-Newton breaks before its first update
# The device may differ from numpy by 4 x the host's spread: both differ from LAPACK only through Jacobi-vs-LAPACK and
# libm-vs-device transcendentals
# The numpy restatement's own pose error against the generator's truth (rotation [rad], translation) for the refine of the true
# inlier set of end_to_end(camera, 0.5) (300 points, 50 % outliers, 0.5 px noise), measured on the CPU and asserted by
# tests/test_mlpnp_cpu.py::test_numpy_error_against_truth; the end-to-end tests allow twice that.  Keys: the camera type
NUMPY_VS_TRUTH = {0: (4.1e-4, 1.3e-3), 1: (5.0e-4, 2.5e-3)}
DEVICE_BOUND = {k: (4 * r, 4 * t) for k, (r, t) in HOST_VS_NUMPY.items()}


@functools.lru_cache(maxsize=None)
def scene(kind: str):
    """kind: "pinhole", "kb8" (general scenes, 0.5 px noise, 50 % outliers) or "planar" (Pinhole, the points on z = 0)."""
    if kind == "planar":
        return sm.make_problem(seed=11, n=300, iterations=N_SETS, camera_type=sm.PINHOLE, plane_z=0.0, inlier_sets=True)
    return sm.make_problem(seed=12, n=300, iterations=N_SETS, camera_type=sm.KB8 if kind == "kb8" else sm.PINHOLE, inlier_sets=True)


@functools.lru_cache(maxsize=None)
def pose_cases():
    """[(kind, "general" / "planar", index array into the scene's correspondences, numpy pose)]: N_SETS minimal sets and the true
    inlier set per scene."""
    cases = []
    for kind in ("pinhole", "kb8", "planar"):
        pb = scene(kind)
        for idx in list(pb.sets) + [np.flatnonzero(pb.inlier).astype(np.int32)]:
            cases.append((kind, "planar" if kind == "planar" else "general", idx, mn.compute_pose(pb.bearing[idx], pb.p3d[idx])))
    return cases


def spread(poses, group):
    """The largest rotation and translation difference of `poses` (one per case, in order) from the numpy poses of the group."""
    rot = trans = 0.0
    for (kind, g, idx, ref), pose in zip(pose_cases(), poses):
        if g == group:
            r, t = mn.pose_difference(pose, ref)
            rot, trans = max(rot, r), max(trans, t)
    return rot, trans


@functools.lru_cache(maxsize=None)
def end_to_end(camera, noise):
    """300 points, 50 % outliers, SetRansacParameters() of the constructor; noise 0: exact bearing vectors."""
    return sm.make_problem(seed=5, n=300, iterations=300, camera_type=camera, outlier_share=0.5, noise_px=noise, exact_bearing=noise == 0.0)
