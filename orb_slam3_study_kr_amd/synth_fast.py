"""Synthetic pyramids for the FAST / IC_Angle part of ORBextractor::ComputeKeyPointsOctTree (osh_orb_fast_detect,
osh_orb_ic_angle): smooth noise with rectangles, blobs and single dots of graded contrast, so that one image holds cells that are
decided at either threshold or stay empty, scores on and next to the thresholds, bright and dark corners, ties between
neighbours, and corners inside the 6-pixel overlap of two cells.  The pyramid is a plain area resampling: how the levels are made
is the caller's business (cv::resize in the reference); the detector only reads them."""
from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass(frozen=True)
class FastFrame:
    pyramid: tuple          # of uint8 [rows, cols] arrays, level 0 first
    ini_th: int = 20
    min_th: int = 7

    @property
    def n_levels(self):
        return len(self.pyramid)


def smooth_noise(rng, h, w, coarse=9, amp=40.0):
    """Bilinear interpolation of a coarse random grid: no corners of its own at the usual thresholds."""
    gh, gw = h // coarse + 2, w // coarse + 2
    g = rng.uniform(-amp, amp, (gh, gw))
    y, x = np.arange(h) / coarse, np.arange(w) / coarse
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    a, b = g[y0][:, x0], g[y0][:, x0 + 1]
    c, d = g[y0 + 1][:, x0], g[y0 + 1][:, x0 + 1]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


def make_image(seed, h, w, density=1.0, fine=2.0, flat_band=True, weak_band=True):
    """An image of h x w: three vertical bands (full contrast, weak contrast, nearly flat) when the flags ask for them."""
    rng = np.random.default_rng(seed)
    img = 128.0 + smooth_noise(rng, h, w)
    contrast = np.ones(w)
    if weak_band:
        contrast[w // 2:] = 0.45
    if flat_band:
        contrast[(5 * w) // 6:] = 0.0
    n = int(density * h * w / 160)
    for _ in range(n):
        kind = rng.integers(0, 4)
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        delta = float(rng.choice([-1, 1]) * rng.integers(3, 60)) * contrast[min(x, w - 1)]
        if kind == 0:      # rectangle
            hh, ww = int(rng.integers(2, 14)), int(rng.integers(2, 14))
            img[y:y + hh, x:x + ww] += delta
        elif kind == 1:    # blob
            r = int(rng.integers(1, 5))
            yy, xx = np.ogrid[-r:r + 1, -r:r + 1]
            m = (yy * yy + xx * xx <= r * r)
            ys, xs = slice(max(y - r, 0), min(y + r + 1, h)), slice(max(x - r, 0), min(x + r + 1, w))
            mm = m[ys.start - (y - r):ys.stop - (y - r), xs.start - (x - r):xs.stop - (x - r)]
            img[ys, xs] += delta * mm
        elif kind == 2:    # single dot
            img[y, x] += delta
        else:              # two equal dots side by side: equal scores next to each other
            img[y, x:x + 2] += delta
    img += rng.normal(0.0, fine, (h, w)) * contrast[None, :]
    if flat_band:
        img[:, (5 * w) // 6:] = np.round(img[:, (5 * w) // 6:].mean())
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def resample(img, rows, cols):
    """Area resampling to rows x cols through an integral image; deterministic integer rounding."""
    h, w = img.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    y0 = (np.arange(rows) * h) // rows
    y1 = np.maximum(((np.arange(rows) + 1) * h + rows - 1) // rows, y0 + 1)
    x0 = (np.arange(cols) * w) // cols
    x1 = np.maximum(((np.arange(cols) + 1) * w + cols - 1) // cols, x0 + 1)
    s = ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]
    area = ((y1 - y0)[:, None] * (x1 - x0)[None, :])
    return ((2 * s + area) // (2 * area)).astype(np.uint8)


def level_sizes(h, w, n_levels, scale=1.2):
    """rows, cols of every level as the reference's ComputePyramid sizes them: cvRound(size * (float)(1 / scale^level))."""
    out, sf = [], np.float32(1.0)
    for l in range(n_levels):
        if l:
            sf = np.float32(sf * np.float32(scale))
        inv = np.float32(1.0) / sf
        out.append((int(np.rint(np.float32(h) * inv)), int(np.rint(np.float32(w) * inv))))
    return out


def make_frame(seed, width=160, height=120, n_levels=1, ini_th=20, min_th=7, **kw) -> FastFrame:
    img = make_image(seed, height, width, **kw)
    pyr = [img] + [resample(img, r, c) for r, c in level_sizes(height, width, n_levels)[1:]]
    return FastFrame(tuple(pyr), ini_th, min_th)


def uniform_frame(side=67, value=90) -> FastFrame:
    return FastFrame((np.full((side, side), value, np.uint8),))


def four_corner_frame(side=67, ini_th=20, min_th=7) -> FastFrame:
    """One isolated dot at each corner of the area in which a side x side level has scores: rows and columns [19, side - 19)."""
    img = np.full((side, side), 60, np.uint8)
    lo, hi = 19, side - 20
    for k, (y, x) in enumerate(((lo, lo), (lo, hi), (hi, lo), (hi, hi))):
        img[y, x] = 60 + (31 + k if k % 2 == 0 else -(31 + k))
    return FastFrame((img,), ini_th, min_th)


def moment_frame():
    """A 128 x 192 level of six 64 x 64 blocks for IC_Angle: uniform (both moments 0), a horizontal ramp up and down (m_01 == 0),
    a vertical ramp up and down (m_10 == 0), a diagonal ramp; with the keypoints at and around the block centres."""
    b = 64
    x = np.arange(b)[None, :].repeat(b, 0)
    y = np.arange(b)[:, None].repeat(b, 1)
    blocks = [np.full((b, b), 77), 40 + 2 * x, 200 - 2 * x, 40 + 2 * y, 200 - 2 * y, 30 + x + 2 * y]
    img = np.zeros((2 * b, 3 * b), np.uint8)
    xy = []
    for k, blk in enumerate(blocks):
        r, c = divmod(k, 3)
        img[r * b:(r + 1) * b, c * b:(c + 1) * b] = blk
        for dy, dx in ((0.0, 0.0), (0.5, -0.5), (-2.5, 1.5), (3.49, -3.5)):   # halves: cvRound goes to the even pixel
            xy.append((c * b + 32 + dx, r * b + 32 + dy))
    return FastFrame((img,)), np.asarray(xy, np.float32), np.zeros(len(xy), np.int32)
