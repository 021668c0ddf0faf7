"""Synthetic loop-candidate problems for the Sim3 RANSAC (osh_orb_sim3_ransac): two keyframe poses in two maps, points seen by both
keyframes, a true Sim3 between the two camera frames with scale 1 or a free scale, noise on the map points worth a given number of
pixels, an outlier share whose second map point lies elsewhere, Pinhole or KannalaBrandt8 for either camera, minimal sets drawn as
data with a least triangle area, and degenerate minimal sets (collinear members, coincident members, a zero denominator of the
scale)."""
from __future__ import annotations

import dataclasses

import numpy as np

from .synth_mlpnp import KB8, KB8_PARAMS, PINHOLE, PINHOLE_PARAMS, project, rodrigues  # noqa: F401 (KB8: for the callers)

F32 = np.float32
CHI2 = 9.210


@dataclasses.dataclass
class Problem:
    camera_type1: int
    camera1: np.ndarray        # [8] float32
    camera_type2: int
    camera2: np.ndarray
    fix_scale: int
    x3dc1: np.ndarray          # [n, 3] float32: mvX3Dc1
    x3dc2: np.ndarray          # [n, 3] float32: mvX3Dc2
    p1im1: np.ndarray          # [n, 2] float32: mvP1im1
    p2im2: np.ndarray          # [n, 2] float32: mvP2im2
    max_error1: np.ndarray     # [n] float32: (float)(size_t)(9.210 * sigma2)
    max_error2: np.ndarray
    sets: np.ndarray           # [iterations, 3] int32
    min_inliers: int = 6
    best_inliers_in: int = 0
    # the truth: X1 = s12 * R12 @ X2 + t12
    R12: np.ndarray = None
    t12: np.ndarray = None
    s12: float = 1.0
    inlier: np.ndarray = None  # [n] bool
    # the scene behind the correspondences (what the class's constructor reads)
    Rcw1: np.ndarray = None    # [3, 3] float32
    tcw1: np.ndarray = None
    Rcw2: np.ndarray = None
    tcw2: np.ndarray = None
    world1: np.ndarray = None  # [n, 3] float32: the points of map 1
    world2: np.ndarray = None
    octave1: np.ndarray = None  # [n] int32
    octave2: np.ndarray = None

    @property
    def n(self) -> int:
        return int(self.x3dc1.shape[0])


def level_sigma2(n_levels: int = 8) -> np.ndarray:
    return (F32(1.2) ** (2 * np.arange(n_levels))).astype(F32)


def truncated_threshold(sigma2) -> np.ndarray:
    """mvnMaxError (a std::vector<size_t>): 9.210 * sigma2 in double, truncated towards zero, as the float the comparison sees."""
    return np.floor(CHI2 * np.asarray(sigma2, F32).astype(np.float64)).astype(np.uint64).astype(F32)


def to_camera(Rcw, tcw, Xw) -> np.ndarray:
    """Rcw * Xw + tcw in float32, ((r0 x + r1 y) + r2 z) + t per row."""
    R, t, X = np.asarray(Rcw, F32), np.asarray(tcw, F32), np.asarray(Xw, F32)
    return np.stack([((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i] for i in range(3)], 1).astype(F32)


def camera(camera_type: int) -> np.ndarray:
    cam = np.zeros(8, F32)
    params = PINHOLE_PARAMS if camera_type == PINHOLE else KB8_PARAMS
    cam[:len(params)] = params
    return cam


def triangle_quality(P) -> float:
    """Area of the triangle of three points over its squared longest side."""
    P = np.asarray(P, np.float64)
    a, b, c = P[1] - P[0], P[2] - P[0], P[2] - P[1]
    longest = max(a @ a, b @ b, c @ c)
    return 0.0 if longest == 0 else 0.5 * np.linalg.norm(np.cross(a, b)) / longest


def draw_sets(x3dc1, x3dc2, iterations: int, rng, min_quality: float = 0.0, pool=None) -> np.ndarray:
    """`iterations` minimal sets of 3 distinct indices (out of `pool`) whose triangles in both cameras have at least min_quality."""
    n = x3dc1.shape[0]
    pool = np.arange(n) if pool is None else np.asarray(pool)
    sets = []
    while len(sets) < iterations:
        s = rng.choice(pool, 3, replace=False)
        if min_quality > 0 and min(triangle_quality(x3dc1[s]), triangle_quality(x3dc2[s])) < min_quality:
            continue
        sets.append(s)
    return np.asarray(sets, np.int32).reshape(-1, 3)


def make_problem(seed: int = 0, n: int = 100, iterations: int = 300, camera_type1: int = PINHOLE, camera_type2: int = PINHOLE,
                 fix_scale: bool = True, outlier_share: float = 0.3, noise_px: float = 0.5, min_inliers: int = 6, min_quality: float = 0.0,
                 inlier_sets: bool = False) -> Problem:
    rng = np.random.RandomState(seed)
    cam1, cam2 = camera(camera_type1), camera(camera_type2)
    # the true Sim3 between the camera frames
    R12 = rodrigues(rng.uniform(-0.25, 0.25, 3))
    t12 = rng.uniform(-0.4, 0.4, 3)
    s12 = 1.0 if fix_scale else float(rng.uniform(0.7, 1.4))
    # points in front of camera 1, and where camera 2 sees them
    half = 1.5 if camera_type1 == PINHOLE else 2.5
    X1 = np.stack([rng.uniform(-half, half, n), rng.uniform(-half * 0.7, half * 0.7, n), rng.uniform(3.0, 7.0, n)], 1)
    X2 = (X1 - t12) @ R12 / s12                      # R12^T (X1 - t12) / s
    # noise on the map points worth noise_px pixels at their depth, in both maps
    f1, f2 = float(cam1[0]), float(cam2[0])
    X1n = X1 + rng.normal(0, 1, (n, 3)) * (noise_px / 3 ** 0.5 * X1[:, 2:3] / f1)
    X2n = X2 + rng.normal(0, 1, (n, 3)) * (noise_px / 3 ** 0.5 * X2[:, 2:3] / f2)
    n_out = int(round(n * outlier_share))
    inlier = np.ones(n, bool)
    out = rng.permutation(n)[:n_out]
    inlier[out] = False
    # an outlier's second map point is another point of the scene: far from where the first one is, in pixels
    if n_out:
        X2n[out] = np.roll(X2[out], 1, 0) + rng.uniform(0.2, 0.5, (n_out, 3)) * rng.choice([-1.0, 1.0], (n_out, 3))
    # the two keyframe poses and the map points behind the camera coordinates
    Rcw1 = rodrigues(rng.uniform(-0.3, 0.3, 3)).astype(F32)
    tcw1 = rng.uniform(-1.0, 1.0, 3).astype(F32)
    Rcw2 = rodrigues(rng.uniform(-0.3, 0.3, 3)).astype(F32)
    tcw2 = rng.uniform(-1.0, 1.0, 3).astype(F32)
    world1 = ((X1n - tcw1.astype(np.float64)) @ Rcw1.astype(np.float64)).astype(F32)
    world2 = ((X2n - tcw2.astype(np.float64)) @ Rcw2.astype(np.float64)).astype(F32)
    x3dc1, x3dc2 = to_camera(Rcw1, tcw1, world1), to_camera(Rcw2, tcw2, world2)
    p1im1 = project(camera_type1, cam1, x3dc1.astype(np.float64)).astype(F32)
    p2im2 = project(camera_type2, cam2, x3dc2.astype(np.float64)).astype(F32)
    octave1, octave2 = rng.randint(0, 4, n).astype(np.int32), rng.randint(0, 4, n).astype(np.int32)
    sigma2 = level_sigma2()
    sets = draw_sets(x3dc1, x3dc2, iterations, rng, min_quality, np.flatnonzero(inlier) if inlier_sets else None)
    return Problem(camera_type1, cam1, camera_type2, cam2, int(fix_scale), x3dc1, x3dc2, p1im1, p2im2, truncated_threshold(sigma2[octave1]),
                   truncated_threshold(sigma2[octave2]), sets, int(min_inliers), 0, R12, t12, s12, inlier, Rcw1, tcw1, Rcw2, tcw2, world1, world2,
                   octave1, octave2)


def with_degenerate_set(pb: Problem, kind: str) -> Problem:
    """A copy whose correspondences 0, 1, 2 form a degenerate minimal set, which becomes iteration 0.  "collinear": the members lie on
    a line in both cameras; "coincident": members 0 and 1 have the same coordinates; "zero_den": the three members coincide in camera
    2, so the rotated relative coordinates are zero and so is the denominator of the scale."""
    x1, x2 = pb.x3dc1.copy(), pb.x3dc2.copy()
    if kind == "collinear":
        for x in (x1, x2):
            x[1] = x[0] + F32(0.5) * (x[2] - x[0])
    elif kind == "coincident":
        x1[1], x2[1] = x1[0], x2[0]
    elif kind == "zero_den":
        x2[1] = x2[2] = x2[0]
    else:
        raise ValueError(kind)
    sets = np.concatenate([np.array([[0, 1, 2]], np.int32), pb.sets]).astype(np.int32)
    return dataclasses.replace(pb, x3dc1=x1, x3dc2=x2, sets=sets)
