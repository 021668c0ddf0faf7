"""Synthetic rectified stereo pairs of images for the calls that extract and match a frame (osh_orb_extract_stereo).

The left image is synth_fast.make_image.  The right image is the left one shifted horizontally by an integer disparity that is
constant inside each of a few horizontal bands (a scene of fronto-parallel planes: xR = xL - d), the columns that come into view
filled with the left image's own reflected content, plus seeded noise of a few grey levels.  The noise makes the SADs of matched
keypoints non-zero: a pair that matches perfectly has median SAD 0 and the median cut then removes every match.
"""
import numpy as np

from . import synth_fast

DISPARITIES = (3, 7, 12)


def make_pair(seed, h, w, disparities=DISPARITIES, noise=3.0, **image_kw):
    """(left, right) uint8 [h, w]: len(disparities) horizontal bands of equal height, band k shifted by disparities[k] pixels."""
    left = synth_fast.make_image(seed, h, w, **image_kw)
    rng = np.random.default_rng(1000003 * seed + 17)
    right = np.empty_like(left)
    edges = np.linspace(0, h, len(disparities) + 1).astype(int)
    for k, d in enumerate(disparities):
        rows = slice(edges[k], edges[k + 1])
        d = int(d)
        right[rows, :w - d] = left[rows, d:]
        right[rows, w - d:] = left[rows, w - d - 1:w - 2 * d - 1:-1] if d else left[rows, :0]
    noisy = right.astype(np.float64) + rng.normal(0.0, noise, (h, w))
    return left, np.clip(np.rint(noisy), 0, 255).astype(np.uint8)


# The named pairs of the tests and the timing script: name -> (seed, rows, cols, n_levels, n_features, bf, image keywords)
PAIRS = {
    "pair_160x120_L3": (3, 120, 160, 3, 300, 40.0, {}),
    "pair_240x180_L4": (5, 180, 240, 4, 500, 40.0, {}),
    "pair_752x480_L8": (31, 480, 752, 8, 1000, 40.0, {}),
}


def named_pair(name):
    """dict(left, right, n_levels, n_features, bf, b) of a named pair; b = 1, so that the largest disparity searched is bf."""
    seed, h, w, n_levels, n_features, bf, kw = PAIRS[name]
    left, right = make_pair(seed, h, w, **kw)
    return dict(left=left, right=right, n_levels=n_levels, n_features=n_features, bf=bf, b=1.0)
