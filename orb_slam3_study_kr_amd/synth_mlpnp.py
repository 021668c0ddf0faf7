"""Synthetic relocalisation problems for the MLPnP RANSAC (osh_orb_mlpnp_solve): world points seen by a Pinhole or KannalaBrandt8
camera at a known pose, pixel noise on the inliers, an outlier share displaced by at least 20 px, an exact-plane option (the world
points on z = plane_z, exactly), and the minimal sets drawn as data."""
from __future__ import annotations

import dataclasses

import numpy as np

PINHOLE, KB8 = 0, 1
PINHOLE_PARAMS = (458.654, 457.296, 367.215, 248.375)
KB8_PARAMS = (190.978, 190.973, 254.932, 256.897, 0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673)
TH2 = 5.991


@dataclasses.dataclass
class Problem:
    camera_type: int
    camera: np.ndarray        # [8] float32
    bearing: np.ndarray       # [n, 3] float64: unproject(p2d) / z
    p3d: np.ndarray           # [n, 3] float64 (float32 values, as GetWorldPos)
    p2d: np.ndarray           # [n, 2] float32
    max_error: np.ndarray     # [n] float32: mvLevelSigma2[octave] * th2
    sets: np.ndarray          # [iterations, 6] int32
    min_inliers: int = 8
    best_inliers_in: int = 0
    best_refine_ok_in: int = 0
    # the truth
    pose: np.ndarray = None   # [12] float64: Rcw row-major, tcw
    inlier: np.ndarray = None  # [n] bool

    @property
    def n(self) -> int:
        return int(self.p3d.shape[0])


def rodrigues(w) -> np.ndarray:
    w = np.asarray(w, np.float64)
    a = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if a < 1e-300:
        return np.eye(3)
    return np.eye(3) + np.sin(a) / a * W + (1 - np.cos(a)) / a ** 2 * (W @ W)


def project(camera_type: int, cam, Xc: np.ndarray) -> np.ndarray:
    """The camera model in float64: [n, 3] camera points -> [n, 2] pixels."""
    cam = np.asarray(cam, np.float64)
    if camera_type == PINHOLE:
        return np.stack([cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]], 1)
    theta = np.arctan2(np.hypot(Xc[:, 0], Xc[:, 1]), Xc[:, 2])
    psi = np.arctan2(Xc[:, 1], Xc[:, 0])
    r = theta + cam[4] * theta ** 3 + cam[5] * theta ** 5 + cam[6] * theta ** 7 + cam[7] * theta ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], 1)


def unproject(camera_type: int, cam, uv: np.ndarray) -> np.ndarray:
    """unproject(kp.pt) / z as the solver's constructor stores it: float32 values in a float64 array, z = 1."""
    cam = np.asarray(cam, np.float64)
    x = (uv[:, 0].astype(np.float64) - cam[2]) / cam[0]
    y = (uv[:, 1].astype(np.float64) - cam[3]) / cam[1]
    if camera_type == KB8:
        theta_d = np.minimum(np.hypot(x, y), np.pi / 2)
        theta = theta_d.copy()
        for _ in range(10):
            t2 = theta * theta
            f = theta * (1 + t2 * (cam[4] + t2 * (cam[5] + t2 * (cam[6] + t2 * cam[7])))) - theta_d
            df = 1 + t2 * (3 * cam[4] + t2 * (5 * cam[5] + t2 * (7 * cam[6] + t2 * 9 * cam[7])))
            theta = theta - f / df
        scale = np.where(theta_d > 1e-8, np.tan(theta) / np.maximum(theta_d, 1e-300), 1.0)
        x, y = x * scale, y * scale
    b = np.stack([x, y, np.ones_like(x)], 1).astype(np.float32)
    return b.astype(np.float64)


def draw_sets(n: int, iterations: int, rng, pool=None) -> np.ndarray:
    """`iterations` minimal sets of 6 distinct indices out of range(n), or out of `pool`."""
    pool = np.arange(n) if pool is None else np.asarray(pool)
    return np.stack([rng.choice(pool, 6, replace=False) for _ in range(iterations)]).astype(np.int32) if iterations else np.zeros((0, 6), np.int32)


def make_problem(seed: int = 0, n: int = 300, iterations: int = 300, camera_type: int = PINHOLE, outlier_share: float = 0.5,
                 noise_px: float = 0.5, plane_z=None, inlier_sets: bool = False, min_inliers=None, exact_bearing: bool = False) -> Problem:
    """exact_bearing: the inliers' bearing vectors are the camera points divided by z in float64 (no pixel rounding), for noise_px = 0."""
    rng = np.random.RandomState(seed)
    cam = np.zeros(8, np.float32)
    params = PINHOLE_PARAMS if camera_type == PINHOLE else KB8_PARAMS
    cam[:len(params)] = params
    R = rodrigues(rng.uniform(-0.15, 0.15, 3))
    t = np.array([0.1, -0.2, 5.0]) + rng.uniform(-0.2, 0.2, 3)
    half = 1.6 if camera_type == PINHOLE else 2.5
    Xw = np.stack([rng.uniform(-half, half, n), rng.uniform(-half * 0.7, half * 0.7, n), rng.uniform(-1.0, 1.0, n)], 1).astype(np.float32)
    if plane_z is not None:
        Xw[:, 2] = np.float32(plane_z)
    Xw = Xw.astype(np.float64)
    Xc = Xw @ R.T + t
    uv = project(camera_type, cam, Xc)
    n_out = int(round(n * outlier_share))
    inlier = np.ones(n, bool)
    inlier[rng.permutation(n)[:n_out]] = False
    # inliers: uniform noise inside a disc of noise_px; outliers: displaced by 20 .. 60 px
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = np.where(inlier, noise_px * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(20.0, 60.0, n))
    p2d = (uv + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)).astype(np.float32)
    octave = rng.randint(0, 4, n)
    max_error = (np.float32(1.2) ** (2 * octave)).astype(np.float32) * np.float32(TH2)
    sets = draw_sets(n, iterations, rng, np.flatnonzero(inlier) if inlier_sets else None)
    if min_inliers is None:
        min_inliers = max(8, int(np.float32(n) * np.float32(0.4)), 6)   # SetRansacParameters() with the constructor's defaults
    bearing = unproject(camera_type, cam, p2d)
    if exact_bearing:
        bearing[inlier] = (Xc / Xc[:, 2:3])[inlier]
    return Problem(camera_type, cam, bearing, Xw, p2d, max_error.astype(np.float32), sets, int(min_inliers), 0, 0,
                   np.concatenate([R.reshape(9), t]), inlier)
