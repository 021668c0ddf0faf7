"""The cases the Sim3 RANSAC tests share (tests/test_sim3_ransac_cpu.py, tests/test_gpu_sim3_ransac.py, the class tests): the size
and camera grids, the hypothesis cases with well-conditioned minimal sets and their numpy references (computed once), the end-to-end
scenes, and the measured bounds."""
import functools

import numpy as np

import sim3_ransac_numpy as s3n
from orb_slam3_study_kr_amd import orb, synth_sim3_ransac as ss

SIZES = (3, 4, 63, 64, 65, 300)          # below, at and above one wavefront of correspondences, and several blocks of 64
ITERATIONS = (1, 3, 300)
CAMERAS = {"pinhole-pinhole": (ss.PINHOLE, ss.PINHOLE), "kb8-kb8": (ss.KB8, ss.KB8), "pinhole-kb8": (ss.PINHOLE, ss.KB8)}

# The minimal sets of the hypothesis cases have a triangle area of at least this share of the squared longest side, in both cameras
MIN_QUALITY = 0.05
HYPOTHESIS_SEEDS = (21, 22, 23, 24)
N_HYPOTHESES = 32
# The largest difference between the host build of csrc/sim3_ransac.h and the numpy restatement over hypothesis_cases(), per float32
# entry relative to the entry's scale (1 for R, the largest |t| entry for t, s for s), measured on the CPU
# (tests/test_sim3_ransac_cpu.py::test_hypotheses_against_numpy prints it): 0.0, every float32 entry of the 128 transforms is equal.
# What could be left is Jacobi against LAPACK rounding in FP64 (about 1e-16), which reaches a float32 entry only when it straddles a
# rounding boundary; on this list it never does.
HOST_VS_NUMPY = 0.0
HYPOTHESIS_BOUND = 4 * HOST_VS_NUMPY

# With equal transforms the Pinhole scoring is the same float32 statements on both sides.  KannalaBrandt8 goes through atan2, cos and
# sin, where two libraries may differ by one float32 unit in theta or psi: 1.2e-7 of an angle of about 1 rad moves a pixel by
# 191 * 1.2e-7 = 2.3e-5 px, an error d^2 with d <= 6 px (the largest threshold is 27) by 2 * 6 * 2.3e-5 = 2.8e-4, which is 3.1e-5 of
# the smallest threshold, 9.  Counts, masks and records are compared when no error lies within this share of its threshold.
THRESHOLD_MARGIN = 1e-4

# End to end: n = 100, 30 % outliers, 0.5 px noise, min_inliers = 15, 300 iterations
END_TO_END_SEEDS = (1, 2, 3, 4)
# The numpy restatement's own error of the hit's transform against the generator's truth over the end-to-end scenes, both scale
# modes: rotation angle [rad], translation [units of the scene], scale [relative], measured on the CPU and asserted by
# tests/test_sim3_ransac_cpu.py::test_end_to_end_numpy_reaches_a_hit; the end-to-end tests allow twice that.  A hit is the first
# record above min_inliers from a minimal set of 3 noisy points, not a refined estimate, so the bound is loose.
NUMPY_VS_TRUTH = (2.75e-2, 1.58e-1, 3.63e-3)
TRUTH_BOUND = tuple(2 * v for v in NUMPY_VS_TRUTH)


@functools.lru_cache(maxsize=None)
def grid_problem(n, iterations, cameras, fix_scale, seed=7):
    c1, c2 = CAMERAS[cameras]
    return ss.make_problem(seed=seed + n, n=n, iterations=iterations, camera_type1=c1, camera_type2=c2, fix_scale=fix_scale,
                           outlier_share=0.3 if n >= 10 else 0.0, min_inliers=min(6, n))


@functools.lru_cache(maxsize=None)
def hypothesis_cases():
    """[(problem, numpy T [N_HYPOTHESES, 13])]: Pinhole scenes, fixed and free scale in turn, sets of at least MIN_QUALITY."""
    cases = []
    for k, seed in enumerate(HYPOTHESIS_SEEDS):
        pb = ss.make_problem(seed=seed, n=60, iterations=N_HYPOTHESES, fix_scale=k % 2 == 0, min_quality=MIN_QUALITY)
        cases.append((pb, s3n.hypotheses(pb)))
    return cases


def hypothesis_difference(T, ref):
    """The largest difference of transforms [k, 13] from the reference, per entry relative to the entry's scale."""
    T, ref = np.asarray(T, np.float64), np.asarray(ref, np.float64)
    scale = np.ones_like(ref)
    scale[:, 9:12] = np.abs(ref[:, 9:12]).max(1, keepdims=True)
    scale[:, 12] = np.abs(ref[:, 12])
    return float((np.abs(T - ref) / scale).max())


@functools.lru_cache(maxsize=None)
def end_to_end(seed, fix_scale):
    return ss.make_problem(seed=seed, n=100, iterations=300, fix_scale=fix_scale, outlier_share=0.3, noise_px=0.5, min_inliers=15)


@functools.lru_cache(maxsize=None)
def end_to_end_numpy(seed, fix_scale):
    return s3n.solve(end_to_end(seed, fix_scale))


def truth_difference(pb, T13):
    """(rotation angle [rad], translation, relative scale) of R, t, s against the generator's truth."""
    T13 = np.asarray(T13, np.float64)
    dR = T13[:9].reshape(3, 3) @ pb.R12.T
    ang = float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return ang, float(np.linalg.norm(T13[9:12] - pb.t12)), float(abs(T13[12] - pb.s12) / pb.s12)


def perturbed(pb, rng, scale):
    """The truth moved by about `scale` (rotation [rad], translation, relative scale)."""
    R = ss.rodrigues(rng.normal(0, scale, 3)) @ pb.R12
    s = pb.s12 * (1.0 + (0.0 if pb.fix_scale else rng.normal(0, scale)))
    return np.concatenate([R.reshape(9), pb.t12 + rng.normal(0, scale, 3), [s]]).astype(np.float32)


def transforms(pb, seed):
    rng = np.random.RandomState(seed)
    truth = np.concatenate([pb.R12.reshape(9), pb.t12, [pb.s12]]).astype(np.float32)
    # a shift along x moves a pixel by f * shift / z, z in [3, 7]: between 0.02 and 0.05 the near points leave before the far ones
    shifted = [truth + np.concatenate([np.zeros(9), [d, 0, 0, 0]]).astype(np.float32) for d in (0.02, 0.03, 0.04)]
    return np.stack([truth] + [perturbed(pb, rng, s) for s in (1e-6, 1e-4, 1e-2, 1e-1)] + shifted + [perturbed(pb, rng, 1.0)])


def mask_bits(mask, n):
    """The flags [.., n] of mask words [.., words], and whether every bit beyond n is 0."""
    bits = orb.mask_bits(mask, 32 * np.shape(mask)[-1])
    return bits[..., :n], not bits[..., n:].any()


def assert_self_consistent(pb, out):
    """The records, first_hit and the best of a result follow from its own counts by the Python scan, and every record's count,
    transform and mask are those of its iteration."""
    want = s3n.scan(out["debug_count"], pb.min_inliers, pb.best_inliers_in)
    n_rec = int(out["n_records"][0])
    assert list(out["record"][:n_rec]) == want["record"] and (out["record"][n_rec:] == -1).all()
    assert int(out["first_hit"][0]) == want["first_hit"]
    assert int(out["best_iteration"][0]) == want["best_iteration"] and int(out["best_count"][0]) == want["best_count"]
    assert np.array_equal(out["record_count"][:n_rec], out["debug_count"][want["record"]]) and not out["record_count"][n_rec:].any()
    assert not out["record_T"][n_rec:].any() and not out["record_mask"][n_rec:].any()
    flags, clean = mask_bits(out["record_mask"], pb.n)
    assert clean
    assert np.array_equal(flags[:n_rec].sum(1), out["record_count"][:n_rec])
    if "debug_T" in out:
        assert np.array_equal(out["record_T"][:n_rec].view(np.uint32), out["debug_T"][want["record"]].view(np.uint32))
