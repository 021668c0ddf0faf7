"""Seeded rectified stereo frames for Frame::ComputeStereoMatches (src/Frame.cc:816-986).

A smoothed-noise scene is rendered into a left and a right ``uint8`` image with a row-dependent sub-pixel disparity
(``right(x, y) = scene(x + d(y), y)``: a point at ``uL`` is seen at ``uR = uL - d(y)``), both get nearest-neighbour pyramids,
and keypoints are placed like an extractor's: integer positions of a level, at least ``MARGIN`` level pixels from its border,
scaled to level 0 by the level's scale factor.  Right keypoints carry position noise, octave jitter and descriptors a few bits
off their left partners'; both sides hold unmatched keypoints.  Switches of ``make_stereo_frame`` build the frames on which the
rare branches of the reference are taken.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

IMG_W, IMG_H = 752, 480
MARGIN = 16            # pixels of a level between its border and the nearest keypoint (ORBextractor's EDGE_THRESHOLD - 3)
SYM_PERIOD = 16        # the symmetric pattern mirrors about every multiple of this column


@dataclass
class StereoFrame:
    left_xy: np.ndarray        # [n_left, 2] float32
    left_octave: np.ndarray    # [n_left] int32
    left_desc: np.ndarray      # [n_left, 32] uint8
    right_xy: np.ndarray
    right_octave: np.ndarray
    right_desc: np.ndarray
    scale_factors: np.ndarray      # [n_levels] float32
    inv_scale_factors: np.ndarray  # [n_levels] float32
    left_pyramid: list             # n_levels 2-D uint8 arrays
    right_pyramid: list
    bf: float
    b: float
    partner: np.ndarray = field(default=None)   # [n_left] index of the right keypoint generated from this one, -1 none

    @property
    def n_levels(self) -> int:
        return len(self.left_pyramid)


def scale_pyramid(n_levels: int, factor: float = 1.2):
    """mvScaleFactor / mvInvScaleFactor as ORBextractor's constructor forms them: a running float32 product and 1.0f / it."""
    sf = np.ones(n_levels, dtype=np.float32)
    for l in range(1, n_levels):
        sf[l] = sf[l - 1] * np.float32(factor)
    return sf, (np.float32(1.0) / sf).astype(np.float32)


def nn_pyramid(img: np.ndarray, sf: np.ndarray, isf: np.ndarray) -> list:
    """Nearest-neighbour levels of cvRound(size * inverse scale) pixels."""
    h, w = img.shape
    out = []
    for l in range(sf.shape[0]):
        wl = int(np.rint(np.float32(w) * isf[l]))
        hl = int(np.rint(np.float32(h) * isf[l]))
        xs = np.minimum((np.arange(wl) * float(sf[l])).astype(np.int64), w - 1)
        ys = np.minimum((np.arange(hl) * float(sf[l])).astype(np.int64), h - 1)
        out.append(np.ascontiguousarray(img[np.ix_(ys, xs)]))
    return out


def _smooth_noise(rng, h, w, passes=3):
    a = rng.random((h, w))
    for _ in range(passes):
        a = (np.roll(a, 1, 1) + 2 * a + np.roll(a, -1, 1)) / 4
        a = (np.roll(a, 1, 0) + 2 * a + np.roll(a, -1, 0)) / 4
    a -= a.min()
    return a / a.max()


def symmetric_rows(rng, h, w):
    """Rows that mirror about every column that is a multiple of SYM_PERIOD: row y is v_y[tri(x)], tri a triangle wave."""
    x = np.arange(w)
    tri = np.abs(((x + SYM_PERIOD) % (2 * SYM_PERIOD)) - SYM_PERIOD)
    v = rng.integers(0, 256, size=(h, SYM_PERIOD + 1), dtype=np.int64)
    return v[:, tri].astype(np.uint8)


def flip_bits(rng, desc: np.ndarray, k: int) -> np.ndarray:
    bits = np.unpackbits(desc)
    idx = rng.choice(256, size=k, replace=False)
    bits[idx] ^= 1
    return np.packbits(bits)


def make_stereo_frame(seed: int, n_left: int = 1500, n_levels: int = 8, width: int = IMG_W, height: int = IMG_H,
                      bf: float = 40.0, b: float = 1.0, low_contrast: bool = False, median_band: bool = False,
                      edge_guard: bool = False, zero_band: bool = False, constant: bool = False,
                      unmatched: float = 0.12, extra_right: float = 0.12, n_right: int | None = None) -> StereoFrame:
    """One frame.  Switches:
    low_contrast  the scene spans a few grey levels: many equal SADs (ties resolved by the first-minimum rule)
    median_band   low contrast everywhere except a band of rows whose right keypoints sit ~7 pixels off (deliberately wrong
                  matches with large SADs): the median cut removes them
    edge_guard    some left keypoints near the left margin have partners a little left of the right image (x < 0, which no
                  extractor produces): the reference's guard at :923.  With the left margin respected the guard cannot fire at
                  the right border (uR <= uL), so this is the only way to take it without leaving an image
    zero_band     a band of rows holds the symmetric pattern with disparity 0 and perfect level-0 keypoints: disparity == 0,
                  the 0.01 branch
    constant      both images are one grey value: every SAD is 0 and the first minimum sits at incR = -5
    n_right       force the number of right keypoints (None: partners + unmatched extras); 0 gives frames without candidates
    """
    rng = np.random.default_rng(seed)
    sf, isf = scale_pyramid(n_levels)
    W, H = width, height
    pad = 64
    scene = _smooth_noise(rng, H, W + pad)
    if constant:
        scene[:] = 0.5
    amp = np.full((H, 1), 255.0)
    band = (int(H * 0.55), int(H * 0.75))
    if low_contrast or median_band:
        amp[:] = 10.0
        if median_band:
            amp[band[0]:band[1]] = 255.0
    scene_u8 = lambda a: np.clip(np.rint(128.0 + (a - 0.5) * amp), 0, 255).astype(np.uint8)
    # disparity of a row: 0.3 px at the top (sub-pixel noise then gives negative disparities) to ~46 px (beyond bf / b) at the bottom
    d_row = 0.3 + 46.0 * (np.arange(H) / H) ** 1.5
    left = scene_u8(scene[:, :W])
    xs = np.arange(W)[None, :] + d_row[:, None]
    x0 = np.floor(xs).astype(np.int64)
    fr = xs - x0
    rows = np.arange(H)[:, None]
    right = scene_u8(scene[rows, x0] * (1 - fr) + scene[rows, np.minimum(x0 + 1, W + pad - 1)] * fr)
    zb = (int(H * 0.2), int(H * 0.3))
    if zero_band:
        pat = symmetric_rows(rng, zb[1] - zb[0], W)
        left[zb[0]:zb[1]] = pat
        right[zb[0]:zb[1]] = pat
        d_row[zb[0]:zb[1]] = 0.0
    lp, rp = nn_pyramid(left, sf, isf), nn_pyramid(right, sf, isf)

    # left keypoints: level by a geometric law, integer level position inside the margin, scaled to level 0
    w_lvl = np.array([0.75 ** l for l in range(n_levels)])
    w_lvl[[lp[l].shape[0] <= 2 * MARGIN + 1 or lp[l].shape[1] <= 2 * MARGIN + 1 for l in range(n_levels)]] = 0.0
    octave = rng.choice(n_levels, size=n_left, p=w_lvl / w_lvl.sum()).astype(np.int32) if n_left else np.zeros(0, np.int32)
    lxy = np.zeros((n_left, 2), dtype=np.float32)
    for i in range(n_left):
        hl, wl = lp[octave[i]].shape
        lxy[i, 0] = np.float32(rng.integers(MARGIN, wl - MARGIN)) * sf[octave[i]]
        lxy[i, 1] = np.float32(rng.integers(MARGIN, hl - MARGIN)) * sf[octave[i]]
    if zero_band and n_left:
        k = min(max(n_left // 20, 4), n_left)           # perfect level-0 keypoints on the symmetric columns of the band
        octave[:k] = 0
        lxy[:k, 0] = rng.integers(2, (W - MARGIN) // SYM_PERIOD, size=k) * SYM_PERIOD
        lxy[:k, 1] = rng.integers(zb[0] + 6, zb[1] - 6, size=k)
    n_edge = min(max(n_left // 20, 4), n_left) if edge_guard else 0
    if n_edge:
        octave[-n_edge:] = 0
        lxy[-n_edge:, 0] = rng.integers(MARGIN, 30, size=n_edge)
        lxy[-n_edge:, 1] = rng.integers(int(H * 0.8), H - MARGIN, size=n_edge)      # rows whose disparity exceeds 30 px
    ldesc = rng.integers(0, 256, size=(n_left, 32), dtype=np.uint8)

    rxy, roct, rdesc = [], [], []
    partner = -np.ones(n_left, dtype=np.int32)
    for i in range(n_left):
        if rng.random() < unmatched:
            continue
        y = float(lxy[i, 1])
        d = float(d_row[min(int(y), H - 1)])
        perfect = zero_band and i < min(max(n_left // 20, 4), n_left)
        o = int(octave[i])
        if not perfect and rng.random() < 0.15:
            o = int(np.clip(o + rng.choice([-1, 1]), 0, n_levels - 1))
        # most partners within a pixel; one in ten a few pixels off, so that the SAD minimum also lands on the window's border
        ux = float(lxy[i, 0]) - d + (0.0 if perfect else rng.normal(0, 0.6 if rng.random() < 0.9 else 4.0))
        uy = y + (0.0 if perfect else rng.normal(0, 0.4))
        if median_band and band[0] <= y < band[1]:
            ux += rng.choice([-7.0, 7.0])
        hl, wl = rp[o].shape
        lim = (MARGIN * float(sf[o]), (wl - MARGIN - 1) * float(sf[o]))
        uy = min(max(uy, MARGIN * float(sf[o])), (hl - MARGIN - 1) * float(sf[o]))
        if i >= n_left - n_edge:
            o, ux = 0, -float(rng.uniform(0.6, 3.0))
        elif not (lim[0] <= ux <= lim[1]):
            continue                                            # its partner would violate the extractor's margin
        nflip = int(rng.integers(0, 40)) if rng.random() < 0.8 else int(rng.integers(60, 120))
        partner[i] = len(rxy)
        rxy.append((ux, uy)); roct.append(o); rdesc.append(flip_bits(rng, ldesc[i], 0 if perfect else nflip))
    n_extra = int(extra_right * n_left)
    for _ in range(n_extra):
        o = int(rng.choice(n_levels, p=w_lvl / w_lvl.sum()))
        hl, wl = rp[o].shape
        rxy.append((float(rng.integers(MARGIN, wl - MARGIN)) * float(sf[o]), float(rng.integers(MARGIN, hl - MARGIN)) * float(sf[o])))
        roct.append(o); rdesc.append(rng.integers(0, 256, size=32, dtype=np.uint8))
    rxy = np.asarray(rxy, dtype=np.float32).reshape(-1, 2)
    roct = np.asarray(roct, dtype=np.int32)
    rdesc = np.asarray(rdesc, dtype=np.uint8).reshape(-1, 32)
    # the extractor's order has nothing to do with the left image's: shuffle
    perm = rng.permutation(rxy.shape[0])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    rxy, roct, rdesc = rxy[perm], roct[perm], rdesc[perm]
    partner = np.where(partner >= 0, inv[np.maximum(partner, 0)] if perm.size else -1, -1).astype(np.int32)
    if n_right is not None:
        if n_right <= rxy.shape[0]:
            rxy, roct, rdesc = rxy[:n_right], roct[:n_right], rdesc[:n_right]
            partner = np.where(partner < n_right, partner, -1).astype(np.int32)
        else:
            m = n_right - rxy.shape[0]
            o = rng.choice(n_levels, size=m, p=w_lvl / w_lvl.sum()).astype(np.int32)
            e = np.zeros((m, 2), dtype=np.float32)
            for k in range(m):
                hl, wl = rp[o[k]].shape
                e[k] = (np.float32(rng.integers(MARGIN, wl - MARGIN)) * sf[o[k]], np.float32(rng.integers(MARGIN, hl - MARGIN)) * sf[o[k]])
            rxy = np.concatenate([rxy, e]); roct = np.concatenate([roct, o])
            rdesc = np.concatenate([rdesc, rng.integers(0, 256, size=(m, 32), dtype=np.uint8)])
    return StereoFrame(np.ascontiguousarray(lxy), octave, ldesc, np.ascontiguousarray(rxy, dtype=np.float32),
                       np.ascontiguousarray(roct, dtype=np.int32), np.ascontiguousarray(rdesc, dtype=np.uint8), sf, isf, lp, rp,
                       float(bf), float(b), partner)


def make_shift_frame(seed: int, shift: int, n: int = 60, width: int = 320, height: int = 240, bf: float = 40.0, b: float = 1.0,
                     constant: bool = False):
    """Known answers: one level; the right image is the left one shifted by `shift` whole pixels (right(x) = left(x + shift)).
    In the upper half the images mirror about every SYM_PERIOD-th column and the first n keypoints sit on those columns with
    identical descriptors, so their SAD minimum is 0 and the two SADs beside it are equal: deltaR == 0.  A frame of such
    keypoints alone has median 0 and the cut removes all of them, so the lower half holds smoothed noise, a few grey levels
    of it changed in the right image, and 4n more keypoints whose SADs are not 0.  constant: both images one grey value.
    Returns (frame, n): the known answers hold for keypoints [0, n)."""
    rng = np.random.default_rng(seed)
    sf, isf = scale_pyramid(1)
    half = height // 2
    wide = symmetric_rows(rng, height, width + 2 * SYM_PERIOD * 4)
    wide[half:] = np.rint(_smooth_noise(rng, height - half, wide.shape[1]) * 255).astype(np.uint8)
    if constant:
        wide[:] = 93
    left = np.ascontiguousarray(wide[:, :width])
    right = np.ascontiguousarray(wide[:, shift:shift + width])
    if not constant:
        right[half:] = np.clip(right[half:].astype(np.int64) + rng.integers(-3, 4, size=right[half:].shape), 0, 255).astype(np.uint8)
    cols = rng.integers(4, width // SYM_PERIOD - 2, size=n) * SYM_PERIOD
    rows_ = rng.permutation(np.arange(MARGIN, half - 6))[:n]           # one keypoint per row
    m = 4 * n
    fill = np.stack([rng.integers(64, width - MARGIN, size=m), rng.integers(half + 6, height - MARGIN, size=m)], axis=1)
    lxy = np.concatenate([np.stack([cols, rows_], axis=1), fill]).astype(np.float32)
    rxy = lxy.copy()
    rxy[:, 0] -= shift
    desc = rng.integers(0, 256, size=(n + m, 32), dtype=np.uint8)
    oct0 = np.zeros(n + m, dtype=np.int32)
    fr = StereoFrame(lxy, oct0, desc, rxy, oct0.copy(), desc.copy(), sf, isf, [left], [right], float(bf), float(b),
                     np.arange(n + m, dtype=np.int32))
    return fr, n
