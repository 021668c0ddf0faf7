"""Synthetic batches for the map point refresh: MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:329-403) and
MapPoint::UpdateNormalAndDepth (:426-494) for the map points of one keyframe (osh_orb_refresh_map_points).

A batch has a table of camera centres (a keyframe has one, a rig keyframe two: left, right) and points with entries in
observation order (ascending keyframe, left before right).  The observation counts come from a skewed distribution (most points
are seen from 2-10 cameras, a long tail reaches 60); about a tenth of the keyframes are bad (use_desc 0), about a fifth are rigs,
and the descriptors of a point are its parent descriptor with a few bits flipped, so rows share their median often and the
"first row with the least median" rule decides.
"""
from __future__ import annotations

import dataclasses

import numpy as np

F = np.float32
SCALE_FACTOR = F(1.2)
N_LEVELS = 8


def scale_factors(n_levels: int = N_LEVELS, factor=SCALE_FACTOR) -> np.ndarray:
    """mvScaleFactors: 1, then repeated float32 multiplication (src/ORBextractor.cc:414-419)."""
    s = np.ones(n_levels, F)
    for level in range(1, n_levels):
        s[level] = s[level - 1] * F(factor)
    return s


@dataclasses.dataclass
class Batch:
    entry_off: np.ndarray     # [P+1] int32
    desc: np.ndarray          # [E, 32] uint8
    centre: np.ndarray        # [E] int32
    use_desc: np.ndarray      # [E] uint8
    centres: np.ndarray       # [C, 3] float32
    pos: np.ndarray           # [P, 3] float32
    ref_centre: np.ndarray    # [P] int32
    level_scale: np.ndarray   # [P] float32
    top_scale: np.ndarray     # [P] float32

    @property
    def n_points(self) -> int:
        return int(self.entry_off.shape[0]) - 1

    @property
    def n_entries(self) -> int:
        return int(self.entry_off[-1])

    def counts(self) -> np.ndarray:
        return np.diff(self.entry_off)


def skewed_counts(rng, n_points: int, top: int = 60) -> np.ndarray:
    """Observation counts: 2 + a geometric body (mean about 5) with one point in twenty from a uniform tail up to `top`."""
    body = 2 + rng.geometric(0.22, n_points) - 1
    tail = rng.integers(20, top + 1, n_points)
    return np.minimum(np.where(rng.random(n_points) < 0.05, tail, body), top).astype(np.int32)


def make_batch(seed: int, n_points: int = 1000, counts=None, n_keyframes: int = 96, bad_fraction: float = 0.1, rig_fraction: float = 0.2,
               max_flips: int = 10) -> Batch:
    """One keyframe's points.  counts: the number of entries per point (default: skewed_counts); a count may exceed the number of
    cameras, the keyframes are then visited again (the entry list of a real point never does, the arithmetic does not care)."""
    rng = np.random.default_rng(seed)
    counts = skewed_counts(rng, n_points) if counts is None else np.asarray(counts, np.int32)
    n_points = int(counts.shape[0])
    rig = rng.random(n_keyframes) < rig_fraction
    bad = rng.random(n_keyframes) < bad_fraction
    first = np.concatenate([[0], np.cumsum(1 + rig.astype(np.int64))]).astype(np.int32)   # the left centre of each keyframe
    n_centres = int(first[-1])
    centres = (rng.normal(0.0, 2.0, (n_centres, 3)) + np.array([0.0, 0.0, -1.0])).astype(F)
    for k in np.flatnonzero(rig):                                                          # the right camera 0.1 m beside the left
        centres[first[k] + 1] = centres[first[k]] + np.array([0.1, 0.002, 0.01], F)
    pos = (rng.normal(0.0, 4.0, (n_points, 3)) + np.array([0.0, 0.0, 12.0])).astype(F)
    levels = scale_factors()
    entry_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    E = int(entry_off[-1])
    desc = np.zeros((E, 32), np.uint8)
    centre = np.zeros(E, np.int32)
    use_desc = np.zeros(E, np.uint8)
    ref_centre = np.zeros(n_points, np.int32)
    for p in range(n_points):
        n = int(counts[p])
        parent = rng.integers(0, 256, 32, dtype=np.uint8)
        e = int(entry_off[p])
        filled = 0
        while filled < n:
            for k in np.sort(rng.choice(n_keyframes, size=min(n - filled, n_keyframes), replace=False)):
                cams = [0, 1] if rig[k] and rng.random() < 0.7 else [int(rng.integers(0, 2))] if rig[k] else [0]
                for cam in cams[: n - filled]:
                    bits = np.unpackbits(parent)
                    flips = rng.choice(256, size=int(rng.integers(0, max_flips + 1)), replace=False)
                    bits[flips] ^= 1
                    desc[e + filled] = np.packbits(bits)
                    centre[e + filled] = first[k] + cam
                    use_desc[e + filled] = 0 if bad[k] else 1
                    filled += 1
                if filled == n:
                    break
        ref_centre[p] = first[int(rng.integers(0, n_keyframes))]
    level_scale = levels[rng.integers(0, N_LEVELS, n_points)]
    top_scale = np.full(n_points, levels[-1], F)
    return Batch(entry_off, desc, centre, use_desc, centres, pos, ref_centre, level_scale, top_scale)


def empty_batch() -> Batch:
    return make_batch(0, counts=np.zeros(0, np.int32))


def edit_point(b: Batch, p: int, desc=None, use_desc=None) -> Batch:
    """A copy of the batch with the descriptors [n, 32] and / or flags [n] of point p replaced."""
    out = dataclasses.replace(b, desc=b.desc.copy(), use_desc=b.use_desc.copy())
    e0, e1 = int(b.entry_off[p]), int(b.entry_off[p + 1])
    if desc is not None:
        out.desc[e0:e1] = np.asarray(desc, np.uint8).reshape(e1 - e0, 32)
    if use_desc is not None:
        out.use_desc[e0:e1] = np.asarray(use_desc, np.uint8)
    return out
