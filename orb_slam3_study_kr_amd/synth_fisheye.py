"""Synthetic frames of a KannalaBrandt8 stereo rig for Frame::ComputeStereoFishEyeMatches (reference src/Frame.cc:1131-1171).

Two 512x512 fisheye cameras with TUM-VI-like intrinsics, a baseline of about 0.1 m and a small relative rotation.  A frame is made
of groups of keypoints, each built to end at one stage of the function:

  true      3D points seen by both cameras: most between 0.3 m and 1.9 m with a parallax cosine below 0.998, `n_far` more up to
            50 m, which the parallax test rejects beyond about 5 m (few, because every cosine from 0.9988 up lies within the
            restatement's relative 1e-3 of the 0.9998 threshold and so counts as borderline), pixel noise growing with the octave,
            the right descriptor a copy of the left one with a few bits flipped
  shared    a second left keypoint on the same point, so one right keypoint is named by two accepted left ones
  decoy     a true pair plus another right keypoint whose descriptor is as close: Lowe's test fails
  wrong     a left keypoint whose descriptor was put on the right keypoint of an unrelated point: negative depths and re-projection
            errors
  reproj1/2 a true pair whose right keypoint is moved off the epipolar curve; with both octaves 0 the left re-projection test fails
            first, with a coarse left octave only the right one fails
  behind2   rays that meet in front of the left camera and behind the right one (needs the right camera ahead of the left: tz > 0)
  tiny      points less than 0.1 mm in front of the left camera (needs the right camera behind the left: tz < 0)
  loose     keypoints with random descriptors on either side
  mono      keypoints outside the overlapping area, in front of mono_left / mono_right

The overlap groups are shuffled, cut or padded with loose keypoints to exactly n_left / n_right, and the mono keypoints put in front.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

IMG = 512
N_LEVELS = 8
SCALE = 1.2
# public TUM-VI calibration (cam0 / cam1 of the 512x512 sequences), rounded
CAM1 = np.array([190.978, 190.973, 254.931, 256.897, 0.0034824, 0.00071503, -0.0020532, 0.00020294], dtype=np.float32)
CAM2 = np.array([190.442, 190.435, 252.598, 254.917, 0.0034003, 0.0017660, -0.0026630, 0.00032995], dtype=np.float32)


@dataclasses.dataclass
class FisheyeFrame:
    left_xy: np.ndarray       # [n_left, 2] float32
    left_octave: np.ndarray   # [n_left] int32
    left_desc: np.ndarray     # [n_left, 32] uint8
    right_xy: np.ndarray
    right_octave: np.ndarray
    right_desc: np.ndarray
    mono_left: int
    mono_right: int
    level_sigma2: np.ndarray  # [n_levels] float32
    cam1: np.ndarray          # [8] float32: fx fy cx cy k1..k4
    cam2: np.ndarray
    precision1: float
    precision2: float
    Rlr: np.ndarray           # [3, 3] float32
    tlr: np.ndarray           # [3] float32
    kind: np.ndarray          # [n_left] the group every left keypoint was built as (a census aid, not an input)


def level_sigma2(n_levels: int = N_LEVELS) -> np.ndarray:
    """mvLevelSigma2 of ORBextractor (src/ORBextractor.cc:418-424): scale factors by repeated float multiplication, squared."""
    sf = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        sf[i] = np.float32(sf[i - 1] * np.float32(SCALE))
    return (sf * sf).astype(np.float32)


def rotation(rotvec) -> np.ndarray:
    w = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def make_rig(tz: float = 0.04, rotvec=(0.010, -0.020, 0.005), baseline: float = 0.1, cam1=CAM1, cam2=CAM2):
    """(cam1, cam2, Rlr, tlr) in float32: x_left = Rlr x_right + tlr, the right camera `baseline` to the right and tz ahead."""
    return (np.asarray(cam1, np.float32), np.asarray(cam2, np.float32), rotation(rotvec).astype(np.float32),
            np.array([baseline, 0.002, tz], np.float32))


def project(cam, X) -> np.ndarray:
    """KannalaBrandt8::project in float64 (src/CameraModels/KannalaBrandt8.cpp:45-63)."""
    cam = np.asarray(cam, np.float64)
    X = np.asarray(X, np.float64)
    th = math.atan2(math.hypot(X[0], X[1]), X[2])
    psi = math.atan2(X[1], X[0])
    t2 = th * th
    r = th * (1 + t2 * (cam[4] + t2 * (cam[5] + t2 * (cam[6] + t2 * cam[7]))))
    return np.array([cam[0] * r * math.cos(psi) + cam[2], cam[1] * r * math.sin(psi) + cam[3]])


def unproject(cam, uv) -> np.ndarray:
    """Unit ray of a pixel in float64 (Newton on the distortion polynomial)."""
    cam = np.asarray(cam, np.float64)
    px, py = (uv[0] - cam[2]) / cam[0], (uv[1] - cam[3]) / cam[1]
    rd = math.hypot(px, py)
    if rd < 1e-12:
        return np.array([0.0, 0.0, 1.0])
    th = rd
    for _ in range(30):
        t2 = th * th
        f = th * (1 + t2 * (cam[4] + t2 * (cam[5] + t2 * (cam[6] + t2 * cam[7])))) - rd
        df = 1 + t2 * (3 * cam[4] + t2 * (5 * cam[5] + t2 * (7 * cam[6] + t2 * 9 * cam[7])))
        th -= f / df
    s = math.sin(th) / rd
    return np.array([px * s, py * s, math.cos(th)])


def _inside(uv, margin=2.0) -> bool:
    return margin <= uv[0] < IMG - margin and margin <= uv[1] < IMG - margin


def _flip(rng, desc, n_bits):
    out = desc.copy()
    for b in rng.choice(256, size=n_bits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make_fisheye_frame(seed: int, n_left: int = 900, n_right: int | None = None, mono_left: int = 40, mono_right: int = 30,
                       tz: float = 0.04, n_far: int = 6, shared: float = 0.05, decoys: float = 0.08, wrong: float = 0.08,
                       reproj: float = 0.06, special: int = 14, loose: float = 0.15, noise: float = 0.25,
                       precision: float = 1e-6) -> FisheyeFrame:
    """One rig frame with exactly n_left / n_right keypoints, mono_left / mono_right of them (at most) in front of the overlap.
    The fractions are of the left keypoints inside the overlap; `special` is the number of behind2 (tz > 0) or tiny (tz < 0) pairs."""
    rng = np.random.default_rng(seed)
    n_right = n_left if n_right is None else n_right
    mono_left, mono_right = min(mono_left, n_left), min(mono_right, n_right)
    cam1, cam2, Rlr, tlr = make_rig(tz)
    R64, t64 = Rlr.astype(np.float64), tlr.astype(np.float64)
    to_right = lambda X: R64.T @ (np.asarray(X, np.float64) - t64)
    sig2 = level_sigma2()
    n_over = n_left - mono_left
    L, R = [], []   # overlap keypoints: (xy, octave, desc[, kind])

    def octave():
        return int(min(N_LEVELS - 1, rng.geometric(0.45) - 1))

    def point(dmin, dmax, max_cos=0.998):
        """A 3D point (left frame) whose projections lie inside both images, its depth log-uniform in [dmin, dmax] and the cosine
        of the angle between its two rays below max_cos (off the baseline's direction the parallax of a near point is small too)."""
        while True:
            uv = rng.uniform(20, IMG - 20, 2)
            if np.hypot(uv[0] - 256, uv[1] - 256) > 235:
                continue
            X = unproject(cam1, uv) * math.exp(rng.uniform(math.log(dmin), math.log(dmax)))
            X2 = to_right(X)
            if X @ (X - t64) / (np.linalg.norm(X) * np.linalg.norm(X - t64)) >= max_cos:
                continue
            if X[2] > 0.05 and X2[2] > 0.05 and _inside(project(cam2, X2)) and np.hypot(*(project(cam2, X2) - 256)) < 240:
                return X

    def observe(X, o1, o2, noisy=True):
        s1, s2 = (noise * SCALE ** o1, noise * SCALE ** o2) if noisy else (0.0, 0.0)
        return project(cam1, X) + rng.normal(0, s1, 2), project(cam2, to_right(X)) + rng.normal(0, s2, 2)

    def new_desc():
        return rng.integers(0, 256, 32, dtype=np.uint8)

    def pair(kind, uv1, uv2, o1, o2, bits=None):
        d = new_desc()
        L.append((uv1, o1, d, kind))
        R.append((uv2, o2, _flip(rng, d, int(rng.integers(0, 7)) if bits is None else bits)))
        return d

    counts = dict(shared=int(shared * n_over), decoy=int(decoys * n_over), wrong=int(wrong * n_over), reproj=int(reproj * n_over),
                  loose=int(loose * n_over))
    n_special = special if n_over >= 200 else 0
    n_far = n_far if n_over >= 200 else 0
    n_true = max(0, n_over - sum(counts.values()) - counts["reproj"] - n_special - n_far)
    for k in range(n_true + n_far):
        X = point(0.3, 1.9) if k < n_true else point(2.2, 50.0, max_cos=2.0)
        o = octave()
        uv1, uv2 = observe(X, o, o)
        d = pair("true", uv1, uv2, o, o)
        if counts["shared"] > 0 and k < n_true and rng.random() < 0.2:
            counts["shared"] -= 1
            L.append((uv1 + rng.normal(0, 0.1, 2), o, _flip(rng, d, 1), "shared"))
    for _ in range(counts["shared"]):
        L.append((rng.uniform(10, IMG - 10, 2), octave(), new_desc(), "loose"))
    for _ in range(counts["decoy"]):
        X = point(0.3, 1.9)
        o = octave()
        uv1, uv2 = observe(X, o, o)
        d = pair("decoy", uv1, uv2, o, o, bits=6)
        R.append((rng.uniform(10, IMG - 10, 2), octave(), _flip(rng, d, int(rng.integers(5, 9)))))
    for _ in range(counts["wrong"]):
        a, b = point(0.3, 1.9), point(0.3, 1.9)
        o = octave()
        pair("wrong", observe(a, o, o)[0], observe(b, o, o)[1], o, o)
    for k in range(2 * counts["reproj"]):
        X = point(0.4, 1.5)
        o1 = 0 if k % 2 == 0 else int(rng.integers(5, N_LEVELS))   # even: the left test fails (-4); odd: only the right one (-5)
        uv1, uv2 = observe(X, 0, 0, noisy=False)
        shift = rng.uniform(9, 13) * (1 if rng.random() < 0.5 else -1)
        pair("reproj1" if k % 2 == 0 else "reproj2", uv1, uv2 + np.array([0.0, shift]), o1, 0)
    made = 0
    while made < n_special:
        if tz > 0:    # the rays meet at X, in front of the left camera and behind the right one: the right keypoint shows -X2
            X = np.array([rng.uniform(0.03, 0.07), rng.uniform(-0.02, 0.02), rng.uniform(0.25, 0.6) * tz])
            X2 = to_right(X)
            if not (X2[2] < -0.2 * tz):
                continue
            uv1, uv2 = project(cam1, X), project(cam2, -X2)
            kind = "behind2"
        else:         # a point closer than 0.1 mm to the left camera, seen far off the axis by the right one
            z = rng.uniform(3e-5, 7e-5)
            X = np.array([rng.uniform(-0.6, 0.6) * z, rng.uniform(-0.6, 0.6) * z, z])
            X2 = to_right(X)
            if not X2[2] > 0.01:
                continue
            uv1, uv2 = project(cam1, X), project(cam2, X2)
            kind = "tiny"
        if _inside(uv1) and _inside(uv2):
            pair(kind, uv1, uv2, 0, 0)
            made += 1
    for _ in range(counts["loose"]):
        L.append((rng.uniform(10, IMG - 10, 2), octave(), new_desc(), "loose"))
        R.append((rng.uniform(10, IMG - 10, 2), octave(), new_desc()))

    def side(items, n, mono, with_kind):
        order = rng.permutation(len(items))
        items = [items[i] for i in order][:n - mono]
        while len(items) < n - mono:
            items.append((rng.uniform(10, IMG - 10, 2), octave(), new_desc(), "loose"))
        head = [(rng.uniform(10, IMG - 10, 2), octave(), new_desc(), "mono") for _ in range(mono)]
        items = head + items
        xy = np.array([it[0] for it in items], np.float32).reshape(-1, 2)
        octv = np.array([it[1] for it in items], np.int32)
        desc = np.array([it[2] for it in items], np.uint8).reshape(-1, 32)
        kind = np.array([it[3] if len(it) > 3 else "" for it in items], dtype=object) if with_kind else None
        return xy, octv, desc, kind

    lxy, loct, ldesc, kind = side(L, n_left, mono_left, True)
    rxy, roct, rdesc, _ = side(R, n_right, mono_right, False)
    return FisheyeFrame(lxy, loct, ldesc, rxy, roct, rdesc, mono_left, mono_right, sig2, cam1, cam2, precision, precision, Rlr, tlr, kind)


def make_pairs_frame(pairs, cam1, cam2, Rlr, tlr, sigma: float = 1.0, precision: float = 1e-6) -> FisheyeFrame:
    """A frame of hand-made keypoint pairs [(uv1, uv2), ...] on a given rig, all octave 0 with level_sigma2 = [sigma]: pair i is
    left i / right i; a far copy of every right descriptor keeps Lowe's test satisfied."""
    rng = np.random.default_rng(len(pairs))
    n = len(pairs)
    ldesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    rdesc = np.concatenate([ldesc, rng.integers(0, 256, (max(n, 2), 32), dtype=np.uint8)])
    lxy = np.array([p[0] for p in pairs], np.float32).reshape(-1, 2)
    rxy = np.concatenate([np.array([p[1] for p in pairs], np.float32).reshape(-1, 2), np.full((max(n, 2), 2), 100.0, np.float32)])
    return FisheyeFrame(lxy, np.zeros(n, np.int32), ldesc, rxy, np.zeros(rxy.shape[0], np.int32), rdesc, 0, 0,
                        np.array([sigma], np.float32), np.asarray(cam1, np.float32), np.asarray(cam2, np.float32), precision, precision,
                        np.asarray(Rlr, np.float32).reshape(3, 3), np.asarray(tlr, np.float32), np.array(["pair"] * n, dtype=object))
