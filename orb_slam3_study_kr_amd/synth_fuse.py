"""Synthetic problems for osh_orb_fuse_search (the search of ORBmatcher::Fuse, src/ORBmatcher.cc:1148-1455, for one map point list
and many target keyframes): the targets, the point list and generators whose points land in, beside and behind the targets."""
from __future__ import annotations

import dataclasses

import numpy as np

PINHOLE, KB8 = 0, 1
CHI2, SIM3 = 0, 1
SKIPPED, BEHIND, OUTSIDE, DISTANCE, ANGLE, EMPTY, SEARCHED = range(7)
NAMES = ("stage", "u", "v", "ur", "level", "radius", "n_candidates", "best_idx", "best_dist")   # the outputs of osh_orb_fuse_search


def same_bits(got, exp):
    """The names of the outputs of two fuse_search results that differ in shape, type or any bit."""
    return [name for name in NAMES
            if got[name].shape != exp[name].shape or got[name].dtype != exp[name].dtype or got[name].tobytes() != exp[name].tobytes()]


@dataclasses.dataclass
class Target:
    """One target keyframe as osh_fuse_target sees it."""
    Rcw: np.ndarray            # [3, 3] float32
    tcw: np.ndarray            # [3]
    Ow: np.ndarray             # [3]
    camera: int = PINHOLE
    fx: float = 256.0
    fy: float = 256.0
    cx: float = 320.0
    cy: float = 240.0
    kb8: tuple = (0.0, 0.0, 0.0, 0.0)
    bf: float = 40.0
    bounds: tuple = (0.0, 640.0, 0.0, 480.0)     # min_x, max_x, min_y, max_y
    grid_min: tuple = (0.0, 0.0)
    cell_inv: tuple = (0.1, 0.1)                 # cell_w_inv, cell_h_inv
    cols: int = 64
    rows: int = 48
    n_levels: int = 8
    scale_factor: float = 1.2
    th: float = 3.0
    key_xy: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros((0, 2), np.float32))
    key_octave: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.int32))
    key_uright: np.ndarray | None = None
    desc: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros((0, 32), np.uint8))

    @property
    def n_keys(self) -> int:
        return int(self.key_octave.shape[0])

    def level_tables(self):
        """mvScaleFactors by repeated float multiplication, mvInvLevelSigma2 = 1 / scale^2, mfLogScaleFactor (src/ORBextractor.cc:424-440)."""
        sf = np.ones(self.n_levels, np.float32)
        for k in range(1, self.n_levels):
            sf[k] = np.float32(sf[k - 1] * np.float32(self.scale_factor))
        inv = (np.float32(1.0) / (sf * sf)).astype(np.float32)
        return sf, inv, np.float32(np.log(np.float64(np.float32(self.scale_factor))))


@dataclasses.dataclass
class Points:
    """The map point list as osh_fuse_points sees it."""
    pos: np.ndarray            # [n, 3] float32
    normal: np.ndarray         # [n, 3]
    min_dist: np.ndarray       # [n]
    max_dist: np.ndarray       # [n]
    desc: np.ndarray           # [n, 32] uint8
    skip: np.ndarray | None = None

    @property
    def n(self) -> int:
        return int(self.min_dist.shape[0])


def rotation(rng, angle):
    """A rotation by up to `angle` radians about a random axis, float32."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-angle, angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K).astype(np.float32)


def make_points(seed: int, n: int, skip_every: int = 0) -> Points:
    """n points in a slab in front of the origin, normals along the viewing ray (MapPoint::UpdateNormalAndDepth) with noise, a distance range around their depth."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-6, 6, n), rng.uniform(-4, 4, n), rng.uniform(-1, 12, n)], axis=1).astype(np.float32)
    normal = pos / np.maximum(np.linalg.norm(pos, axis=1, keepdims=True), 1e-3) + rng.normal(scale=0.45, size=(n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    depth = np.linalg.norm(pos, axis=1)
    max_dist = (depth * rng.uniform(0.9, 4.0, n)).astype(np.float32)
    min_dist = (max_dist / np.float32(1.2 ** 7) * rng.uniform(0.8, 1.6, n)).astype(np.float32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    skip = None
    if skip_every:
        skip = (np.arange(n) % skip_every == skip_every - 1).astype(np.uint8)
    return Points(pos, normal, min_dist, max_dist, desc, skip)


def approx_project(t: Target, pos):
    """Float64 projection of world points into the target (for placing keypoints, not for checking): uv [n, 2], depth [n]."""
    pc = pos.astype(np.float64) @ t.Rcw.astype(np.float64).T + t.tcw.astype(np.float64)
    z = pc[:, 2]
    with np.errstate(all="ignore"):
        if t.camera == KB8:
            r_xy = np.hypot(pc[:, 0], pc[:, 1])
            theta = np.arctan2(r_xy, z)
            psi = np.arctan2(pc[:, 1], pc[:, 0])
            k = t.kb8
            r = theta + k[0] * theta ** 3 + k[1] * theta ** 5 + k[2] * theta ** 7 + k[3] * theta ** 9
            uv = np.stack([t.fx * r * np.cos(psi) + t.cx, t.fy * r * np.sin(psi) + t.cy], axis=1)
        else:
            uv = np.stack([t.fx * pc[:, 0] / z + t.cx, t.fy * pc[:, 1] / z + t.cy], axis=1)
    return uv, z


def make_target(seed: int, points: Points, n_keys: int, camera: int = PINHOLE, stereo: bool = False, th: float = 3.0, away: bool = False,
                cluster: int = 0) -> Target:
    """A target near the origin looking down +z (away: down -z from 20 m behind the points, so that no point passes) with n_keys keypoints, most of them a
    pixel or two from the projection of a point and with a descriptor a few bits from it, at an octave around the one the point
    predicts.  stereo: key_uright with about a third negative.  cluster: that many of the keypoints on one spot (one grid cell)."""
    rng = np.random.default_rng(seed)
    R = rotation(rng, 0.15)
    if away:
        R = (np.diag([1.0, -1.0, -1.0]) @ R).astype(np.float32)
    centre = rng.uniform(-0.5, 0.5, 3).astype(np.float32)
    if away:
        centre[2] -= np.float32(20.0)   # every point of make_points is behind it
    tcw = (-(R.astype(np.float64) @ centre.astype(np.float64))).astype(np.float32)
    t = Target(Rcw=R, tcw=tcw, Ow=centre, camera=camera, th=th)
    if camera == KB8:
        t.fx, t.fy, t.kb8, t.bf = 190.0, 190.5, (-0.0034, 0.0007, -0.002, 0.0002), 0.0
    key_xy = np.stack([rng.uniform(-20, 660, n_keys), rng.uniform(-20, 500, n_keys)], axis=1)
    key_octave = rng.integers(0, t.n_levels, n_keys)
    desc = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    disparity = rng.uniform(2, 30, n_keys)
    if points.n and n_keys:
        uv, z = approx_project(t, points.pos)
        dist = np.linalg.norm(points.pos.astype(np.float64) - centre, axis=1)
        with np.errstate(all="ignore"):
            level = np.clip(np.ceil(np.log(points.max_dist / dist) / np.log(t.scale_factor)), 0, t.n_levels - 1)
        ok = np.flatnonzero((z > 0) & np.isfinite(uv).all(axis=1) & (uv[:, 0] > 0) & (uv[:, 0] < 640) & (uv[:, 1] > 0) & (uv[:, 1] < 480))
        for k in range(0, n_keys, 4 if n_keys > 8 else 1):   # every fourth keypoint stays random
            if ok.size == 0:
                break
            for j in range(k, min(k + (3 if n_keys > 8 else 1), n_keys)):
                p = ok[rng.integers(ok.size)]
                key_xy[j] = uv[p] + rng.normal(scale=1.5, size=2)
                disparity[j] = t.bf / z[p] + rng.normal(scale=1.0)
                key_octave[j] = int(np.clip(level[p] - rng.integers(0, 3) + 1, 0, t.n_levels - 1))
                d = points.desc[p].copy()
                flips = rng.integers(0, 256, rng.integers(0, 40))
                for b in flips:
                    d[b >> 3] ^= np.uint8(1 << (b & 7))
                desc[j] = d
    if cluster:
        spot = key_xy[0].copy() if n_keys else np.zeros(2)
        spot = np.clip(spot, 15, 400)
        key_xy[:cluster] = spot + rng.uniform(-0.4, 0.4, (cluster, 2))
    t.key_xy = key_xy.astype(np.float32)
    t.key_octave = key_octave.astype(np.int32)
    t.desc = desc
    if stereo:
        ur = t.key_xy[:, 0] - disparity.astype(np.float32)
        ur[rng.uniform(size=n_keys) < 0.33] = -1.0
        t.key_uright = ur.astype(np.float32)
    return t


def make_case(seed: int, n_targets: int, n_points: int, keys, camera: int = PINHOLE, stereo: bool = False, th: float = 3.0,
              skip_every: int = 0, away=(), cluster=None):
    """n_targets targets (keys: keypoints per target, one number or a list), one list of n_points points.  away: targets that look
    the other way; cluster: {target: keypoints on one spot}."""
    points = make_points(seed, n_points, skip_every)
    keys = [keys] * n_targets if np.isscalar(keys) else list(keys)
    targets = [make_target(seed * 1000 + k, points, keys[k], camera, stereo, th, k in away, (cluster or {}).get(k, 0)) for k in range(n_targets)]
    return targets, points
