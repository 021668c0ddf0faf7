"""The blur and the steered-BRIEF descriptor of ORBextractor::operator() restated in numpy from their definitions
(include/orbslam3_hip.h, "blur and steered-BRIEF descriptors"): what tests/test_brief_cpu.py and tests/test_gpu_brief.py compare the
host build and the kernels with, bit for bit.  It shares no code with csrc/orb_brief.h: the blur is two reflect-padded correlations
in int64, cos and sin come from math rounded to float32, the offsets are float32 array operations with np.rint.

Also the committed cases: seeded tables, crafted tables and angles, and the census items they are there for."""
import functools
import math

import numpy as np

from orb_slam3_study_kr_amd import synth_fast as sf

F = np.float32
FACTOR_PI = F(math.pi / 180.0)
# found by a seeded search over random float32 angles and the 26 x 26 table grid (2 * 10^7 samples sufficed): at these, the x offset
# of the point is -10 / +10 in the unfused form and -9 / +9 when the first product is fused into the difference (for the first
# case also when the second one is)
FMA_CASES = ((F(10.23166561126709), (-12, -13)), (F(96.3818588256836), (-5, -9)))


def default_weights(ksize=7, sigma=2.0):
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) // 2
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    k = k / k.sum() * 256.0
    out, carry = np.zeros(ksize, np.int64), 0.0
    for i in range(ksize // 2):
        want = k[i] + carry
        q = int(np.rint(want))
        carry = want - q
        out[i] = out[ksize - 1 - i] = q
    out[ksize // 2] = 256 - out.sum()
    return out


def blur(level, w=None):
    """B of the level [rows, cols] uint8 with the weights w (None: the default)."""
    w = default_weights() if w is None else np.asarray(w, np.int64)
    rows, cols = level.shape
    p = np.pad(level.astype(np.int64), ((0, 0), (3, 3)), mode="reflect")
    h = sum(w[u] * p[:, u:u + cols] for u in range(7))
    assert h.max() <= 65280
    p = np.pad(h, ((3, 3), (0, 0)), mode="reflect")
    return ((sum(w[v] * p[v:v + rows, :] for v in range(7)) + 32768) >> 16).astype(np.uint8)


def rotation(angle):
    """cos_sin [n, 2] float32 of the angles (degrees, float32)."""
    rad = (np.asarray(angle, F) * FACTOR_PI).astype(F)
    return np.asarray([[F(math.cos(float(r))), F(math.sin(float(r)))] for r in rad], F).reshape(-1, 2)


def offsets(cos_sin, pattern):
    """dx, dy [n, 512] int of every table point for every keypoint."""
    a, b = cos_sin[:, 0:1], cos_sin[:, 1:2]
    px, py = pattern[None, :, 0].astype(F), pattern[None, :, 1].astype(F)
    dx = np.rint((px * a).astype(F) - (py * b).astype(F))
    dy = np.rint((px * b).astype(F) + (py * a).astype(F))
    return dx.astype(np.int64), dy.astype(np.int64)


def reach(pattern):
    r2 = int((pattern.astype(np.int64) ** 2).sum(axis=1).max())
    return next(R for R in range(32) if R * R >= r2)


def describe(pyramid, xy, level, angle, pattern, w=None):
    """The expected outputs of one osh_orb_describe frame: descriptors [n, 32], cos_sin [n, 2], blurred (every level with at least
    4 rows and columns, None for the others), and for the census samples [n, 512], dx, dy."""
    pattern = np.asarray(pattern, np.int64).reshape(512, 2)
    xy = np.asarray(xy, F).reshape(-1, 2)
    level = np.asarray(level, np.int64)
    blurred = [blur(p, w) if min(p.shape) >= 4 else None for p in pyramid]
    cs = rotation(angle)
    dx, dy = offsets(cs, pattern)
    cx, cy = np.rint(xy[:, 0]).astype(np.int64), np.rint(xy[:, 1]).astype(np.int64)
    samples = np.zeros((len(level), 512), np.int64)
    for l in sorted(set(level.tolist())):
        m = level == l
        yy, xx = cy[m, None] + dy[m], cx[m, None] + dx[m]
        assert yy.min() >= 0 and xx.min() >= 0 and yy.max() < pyramid[l].shape[0] and xx.max() < pyramid[l].shape[1], "a sample leaves its level"
        samples[m] = blurred[l][yy, xx]
    bits = samples[:, 0::2] < samples[:, 1::2]
    desc = np.packbits(bits, axis=1, bitorder="little") if len(level) else np.zeros((0, 32), np.uint8)
    return dict(descriptors=desc, cos_sin=cs, blurred=blurred, samples=samples, dx=dx, dy=dy)


def assert_same(got, exp, what, debug=True):
    """Stage by stage, so that a failure names its stage."""
    if debug:
        for l, (g, e) in enumerate(zip(got["blurred"], exp["blurred"])):
            if e is not None:
                bad = np.argwhere(g != e)
                assert not len(bad), f"{what}: blurred level {l} differs at {len(bad)} pixels, first (y, x) = {bad[0].tolist()}: {g[tuple(bad[0])]} != {e[tuple(bad[0])]}"
        assert np.array_equal(got["cos_sin"].view(np.uint32), exp["cos_sin"].view(np.uint32)), f"{what}: cos_sin"
    bad = np.argwhere((got["descriptors"] != exp["descriptors"]).any(axis=1)).ravel()
    assert not len(bad), f"{what}: {len(bad)} of {len(exp['descriptors'])} descriptors differ, first keypoint {bad[0]}"


# ---- tables

def seeded_table(seed):
    """512 points in [-13, 12]^2, the first one the farthest there is: reach 19 like the reference's table."""
    t = np.random.default_rng(seed).integers(-13, 13, (512, 2)).astype(np.int8)
    t[0] = (-13, -13)
    return t


def crafted_table():
    """A seeded table whose first pairs are the census's: points (odd, 0) and (0, odd) for offsets on k + 0.5, the points of FMA_CASES,
    a pair of equal points (equal samples)."""
    t = seeded_table(77)
    odd = [(1, 0), (3, 0), (5, 0), (7, 0), (9, 0), (11, 0), (0, 1), (0, 3), (0, 5), (0, 7), (-1, 0), (-3, 0), (0, -5), (0, -7)]
    for k, p in enumerate(odd):
        t[2 + k] = p
    t[16], t[17] = FMA_CASES[0][1], FMA_CASES[1][1]
    t[18] = t[19] = (4, -6)
    return t


CRAFTED_ANGLES = np.asarray([0.0, 90.0, 180.0, 270.0, 30.0, 60.0, 45.0, 135.0, 225.0, 315.0, FMA_CASES[0][0], FMA_CASES[1][0], 359.99, 12.5, 101.25,
                             200.0625, 299.9], F)


# ---- levels and cases

def noise_level(seed, rows, cols):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols)).astype(np.uint8)


def checkerboard(rows, cols):
    y, x = np.mgrid[0:rows, 0:cols]
    return (((x + y) & 1) * 255).astype(np.uint8)


def grid_keypoints(seed, shapes, R, per_level, levels=None):
    """per_level random legal keypoints on each of `levels` (default all that can hold one), the four extreme ones first; fractional
    coordinates, angles over the whole circle."""
    rng = np.random.default_rng(seed)
    xy, lv = [], []
    for l, (rows, cols) in enumerate(shapes):
        if (levels is not None and l not in levels) or rows < 2 * R + 1 or cols < 2 * R + 1:
            continue
        pts = [(R, R), (cols - 1 - R, R), (R, rows - 1 - R), (cols - 1 - R, rows - 1 - R)]
        for _ in range(per_level):
            # rounded centres in [R, size - 1 - R]: uniform on [R - 0.49, size - 1 - R + 0.49]
            pts.append((rng.uniform(R - 0.49, cols - 1 - R + 0.49), rng.uniform(R - 0.49, rows - 1 - R + 0.49)))
        xy += pts
        lv += [l] * len(pts)
    xy = np.asarray(xy, F).reshape(-1, 2)
    angle = rng.uniform(0, 360, len(lv)).astype(F)
    return xy, np.asarray(lv, np.int32), angle


def _case(name):
    """name -> dict(pyramid, xy, level, angle, pattern, blur_q8)."""
    w = None
    if name == "one_39x39":                       # the one legal keypoint of the smallest level
        pyr, pattern = (noise_level(1, 39, 39),), seeded_table(1)
        xy, level, angle = np.asarray([[19, 19]], F), np.zeros(1, np.int32), np.asarray([33.0], F)
    elif name == "extremes_45x52":                # rows 45, cols 52: the four extreme legal positions, at every crafted angle
        pyr, pattern = (noise_level(2, 45, 52),), crafted_table()
        pts = [(19, 19), (32, 19), (19, 25), (32, 25)]
        xy = np.asarray([p for p in pts for _ in CRAFTED_ANGLES], F)
        angle = np.tile(CRAFTED_ANGLES, len(pts))
        level = np.zeros(len(xy), np.int32)
    elif name == "edges_60x70":                   # the farthest point (-13, -13), direction 225 degrees, turned onto each edge
        pyr, pattern = (noise_level(3, 60, 70),), seeded_table(3)
        xy = np.asarray([(19, 30), (50, 30), (35, 19), (35, 40)], F)          # 19 from the left, right, top, bottom edge
        angle = np.asarray([315.0, 135.0, 45.0, 225.0], F)                     # 225 + angle = 180, 0, 270, 90
        level = np.zeros(4, np.int32)
    elif name.startswith("tile_"):                # sizes around the 64 x 16 blur tile: rows x cols
        rows, cols = (int(v) for v in name[5:].split("x"))
        pyr, pattern = (noise_level(rows * 1000 + cols, rows, cols),), seeded_table(4)
        xy, level, angle = grid_keypoints(5, [(rows, cols)], 19, 6)
    elif name in ("const_255", "const_0", "checker"):
        img = {"const_255": np.full((41, 47), 255, np.uint8), "const_0": np.zeros((41, 47), np.uint8), "checker": checkerboard(41, 47)}[name]
        pyr, pattern = (img,), seeded_table(6)
        xy, level, angle = grid_keypoints(6, [img.shape], 19, 4)
    elif name == "pyramid_120x90":                # 3 levels, keypoints on levels 0 and 2 only
        f = sf.make_frame(11, width=120, height=90, n_levels=3)
        pyr, pattern = f.pyramid, seeded_table(7)
        xy, level, angle = grid_keypoints(7, [p.shape for p in pyr], 19, 12, levels=(0, 2))
    elif name == "identity_weights":
        pyr, pattern, w = (noise_level(8, 50, 67),), seeded_table(8), np.asarray([0, 0, 0, 256, 0, 0, 0], np.uint16)
        xy, level, angle = grid_keypoints(8, [(50, 67)], 19, 8)
    elif name == "asymmetric_weights":
        pyr, pattern, w = (noise_level(9, 50, 67),), seeded_table(9), np.asarray([1, 2, 3, 4, 5, 6, 235], np.uint16)
        xy, level, angle = grid_keypoints(9, [(50, 67)], 19, 8)
    elif name == "reach_22":                      # the largest table the entry takes
        pattern = np.random.default_rng(10).integers(-15, 16, (512, 2)).astype(np.int8)
        pattern[0] = (15, -15)
        pyr = (noise_level(10, 47, 81),)
        xy, level, angle = grid_keypoints(10, [(47, 81)], 22, 10)
    elif name == "vga_752x480_L8":
        f = sf.make_frame(21, width=752, height=480, n_levels=8)
        pyr, pattern = f.pyramid, seeded_table(12)
        xy, level, angle = grid_keypoints(12, [p.shape for p in pyr], 19, 150)
    else:
        raise KeyError(name)
    return dict(pyramid=tuple(pyr), xy=xy, level=level, angle=angle, pattern=pattern, blur_q8=w)


# the 64 x 16 tile: exactly one (rows 16 cannot hold a keypoint, so one tile is blur-only), exactly two in each direction, seams
# crossed with remainders in both directions
TILE_CASES = ["tile_39x64", "tile_48x64", "tile_39x128", "tile_41x70", "tile_50x131", "tile_65x129"]
CASE_NAMES = ["one_39x39", "extremes_45x52", "edges_60x70"] + TILE_CASES + ["const_255", "const_0", "checker", "pyramid_120x90", "identity_weights",
                                                                          "asymmetric_weights", "reach_22"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(item for OrbMatcher.describe, expected outputs); computed once and shared: leave both unchanged."""
    it = _case(name)
    exp = describe(it["pyramid"], it["xy"], it["level"], it["angle"], it["pattern"], it["blur_q8"])
    return it, exp


def item(name, **replace):
    it = dict(case(name)[0])
    it.update(replace)
    return it
