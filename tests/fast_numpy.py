"""A vectorised numpy restatement of the integer part of ORBextractor::ComputeKeyPointsOctTree (reference
src/ORBextractor.cc:781-896), written from the definitions and sharing no code with csrc/orb_fast.h: the cell geometry of a level,
cv::FAST(..., threshold, true) as "nine contiguous circle pixels brighter than v + t or darker than v - t" with the score as the
largest such t, the 3x3 strict maximum inside a cell's sub-image, the two-threshold rule, and IC_Angle with OpenCV's documented
scalar fastAtan2 in float32.  The score of a pixel depends on its 7x7 neighbourhood alone, so it is computed once per level and a
cell takes the part that lies at least 3 pixels inside its sub-image."""
import functools

import numpy as np

from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_fast as sf

F = np.float32
# the Bresenham circle of radius 3, clockwise from the bottom: (dx, dy)
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3))


def geometry(rows, cols):
    """nCols, nRows, wCell, hCell, maxBorderX, maxBorderY in the reference's float32 / int steps (0 cells: the defined skip)."""
    max_x, max_y = cols - 16, rows - 16
    width, height = F(max_x - 16), F(max_y - 16)
    n_cols, n_rows = int(width / F(35)), int(height / F(35))
    if n_cols <= 0 or n_rows <= 0:
        return 0, 0, 0, 0, max_x, max_y
    return n_cols, n_rows, int(np.ceil(width / F(n_cols))), int(np.ceil(height / F(n_rows))), max_x, max_y


def cells(rows, cols):
    """(i, j, x0, y0, w, h) of every existing cell in (i, j) order."""
    n_cols, n_rows, w_cell, h_cell, max_x, max_y = geometry(rows, cols)
    out = []
    for i in range(n_rows):
        ini_y = 16 + i * h_cell
        if ini_y >= max_y - 3:
            continue
        for j in range(n_cols):
            ini_x = 16 + j * w_cell
            if ini_x >= max_x - 6:
                continue
            out.append((i, j, ini_x, ini_y, min(ini_x + w_cell + 6, max_x) - ini_x, min(ini_y + h_cell + 6, max_y) - ini_y))
    return out


def level_scores(img):
    """Per pixel at least 3 inside the image: score, polarity of the best arc (+1 brighter, -1 darker) and its first circle index;
    0 elsewhere.  score = max over arcs of min over the arc of |difference in the arc's direction|, minus 1, not below 0."""
    h, w = img.shape
    score = np.zeros((h, w), np.int32)
    pol = np.zeros((h, w), np.int8)
    start = np.zeros((h, w), np.int8)
    if h < 7 or w < 7:
        return score, pol, start
    a = img.astype(np.int32)
    centre = a[3:h - 3, 3:w - 3]
    d = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - centre for dx, dy in CIRCLE])          # [16, H, W]
    ring = np.concatenate([d, d[:8]])                                                               # arcs may wrap past index 15
    bright = np.stack([ring[s:s + 9].min(0) for s in range(16)])
    dark = np.stack([(-ring[s:s + 9]).min(0) for s in range(16)])
    both = np.concatenate([bright, dark])                                                           # [32, H, W]
    best = both.argmax(0)
    val = both.max(0) - 1
    score[3:h - 3, 3:w - 3] = np.maximum(val, 0)
    pol[3:h - 3, 3:w - 3] = np.where(best < 16, 1, -1)
    start[3:h - 3, 3:w - 3] = best % 16
    return score, pol, start


def cell_kept(score, x0, y0, w, h):
    """The score map of the sub-image (0 outside [3, size - 3)), the mask of pixels that are positive and strictly greater than
    their eight neighbours, and the mask of positive pixels that no neighbour beats but one equals, all [h, w]."""
    s = np.zeros((h + 2, w + 2), np.int32)
    if h > 6 and w > 6:
        s[4:h - 2, 4:w - 2] = score[y0 + 3:y0 + h - 3, x0 + 3:x0 + w - 3]
    c = s[1:-1, 1:-1]
    kept = c > 0
    unbeaten, equalled = c > 0, np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                nb = s[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
                kept &= c > nb
                unbeaten &= c >= nb
                equalled |= c == nb
    return c, kept, unbeaten & equalled


def detect(frame):
    """What osh_orb_fast_detect returns for one frame, plus what the census looks at."""
    xy, resp, level, cell, used, level_count = [], [], [], [], [], []
    census = dict(tie=0, scores=set(), pol=set(), wrap=0, twice=0, edge_pairs=0)
    for l, img in enumerate(frame.pyramid):
        rows, cols = img.shape
        score, pol, start = level_scores(img)
        n_cols, n_rows, w_cell, h_cell, _, _ = geometry(rows, cols)
        n_level = 0
        emitted = {}      # absolute pixel -> the cells that emitted it
        for i, j, x0, y0, w, h in cells(rows, cols):
            c, kept, tied = cell_kept(score, x0, y0, w, h)
            at_ini, at_min = kept & (c >= frame.ini_th), kept & (c >= frame.min_th)
            chosen = at_ini if at_ini.any() else at_min
            used.append(capi.OSH_FAST_AT_INI if at_ini.any() else capi.OSH_FAST_AT_MIN if at_min.any() else capi.OSH_FAST_EMPTY)
            ys, xs = np.nonzero(chosen)            # row-major
            n_level += len(ys)
            xy.append(np.stack([xs + j * w_cell, ys + i * h_cell], 1).astype(F))
            resp.append(c[ys, xs].astype(F))
            level.append(np.full(len(ys), l, np.int32))
            cell.append(np.full(len(ys), len(used) - 1, np.int32))
            # census
            census["scores"].update(int(v) for v in c[kept])          # of every strict local maximum, emitted or not
            census["pol"].update(int(v) for v in pol[y0 + ys, x0 + xs])
            census["wrap"] += int((start[y0 + ys, x0 + xs] > 7).sum())
            census["tie"] += int((tied & (c >= frame.min_th)).sum())   # adjacent pixels of equal score, each suppressed by the other alone
            for y, x in zip(ys, xs):
                emitted.setdefault((y0 + y, x0 + x), []).append(len(used) - 1)
        # the areas in which neighbouring cells have scores tile the level, so no pixel can come from two cells; what the 6-pixel
        # overlap does is cut a neighbourhood: two adjacent pixels, each the maximum of its own cell, are both emitted although
        # the stronger would have suppressed the weaker in an undivided image
        for (y, x), who in emitted.items():
            census["twice"] += len(who) > 1
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = emitted.get((y + dy, x + dx))
                    if (dy or dx) and q and q[0] != who[0] and score[y + dy, x + dx] >= score[y, x]:
                        census["edge_pairs"] += 1
        level_count.append(n_level)
    cat = lambda parts, dt, shape: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
    return dict(level_count=np.asarray(level_count, np.int32), xy=cat(xy, F, (0, 2)).reshape(-1, 2), response=cat(resp, F, (0,)),
                level=cat(level, np.int32, (0,)), cell=cat(cell, np.int32, (0,)), used_min_th=np.asarray(used, np.uint8),
                census=census)


def disc():
    """The 31 x 31 mask of the patch IC_Angle sums over: the disc of radius 15, |u| <= round(sqrt(15^2 - v^2)), taken from the rows
    below the diagonal (|v| <= 15 / sqrt 2) and mirrored about the diagonal for the rest, which is what makes it symmetric."""
    vv, uu = np.mgrid[-15:16, -15:16]
    below = (np.abs(uu) <= np.rint(np.sqrt(225.0 - vv * vv))) & (np.abs(vv) <= int(15 / np.sqrt(2.0)))
    return below | below.T


def fast_atan2(y, x):
    """OpenCV's scalar fastAtan2 on float32 arrays, one float32 operation per step."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    s = F(180.0 / np.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * s, F(-0.3258083974640975) * s, F(0.1555786518463281) * s, F(-0.04432655554792128) * s
    eps = F(np.finfo(np.float64).eps)
    ax, ay = np.abs(x), np.abs(y)
    first = ax >= ay
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(first, ay / (ax + eps), ax / (ay + eps)).astype(F)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(first, a, F(90) - a).astype(F)
    a = np.where(x < 0, F(180) - a, a).astype(F)
    a = np.where(y < 0, F(360) - a, a).astype(F)
    return a


def ic_angle(pyramid, xy, level):
    """m10, m01, angle of keypoints (xy in the pixels of their level)."""
    vv, uu = np.mgrid[-15:16, -15:16]
    mask = disc()
    assert ((mask.sum(1)[15:] - 1) // 2).tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]   # the row half-widths
    n = len(level)
    m10, m01 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    cx, cy = np.rint(np.asarray(xy, F)[:, 0]).astype(int), np.rint(np.asarray(xy, F)[:, 1]).astype(int)   # halves to even
    for i in range(n):
        patch = pyramid[level[i]][cy[i] - 15:cy[i] + 16, cx[i] - 15:cx[i] + 16].astype(np.int64)
        assert patch.shape == (31, 31)
        m10[i] = (patch * uu * mask).sum()
        m01[i] = (patch * vv * mask).sum()
    return dict(m10=m10, m01=m01, angle=fast_atan2(m01.astype(F), m10.astype(F)))


# ---- the committed cases: name -> frame.  Seeds were picked on the CPU until the census of test_fast_cpu.py held.
def _cases():
    c = {}
    c["mix_160x120"] = sf.make_frame(3, 160, 120, 3)
    c["mix_240x180_low_th"] = sf.make_frame(5, 240, 180, 4, ini_th=12, min_th=5)
    c["dense_200x150"] = sf.make_frame(7, 200, 150, 2, density=3.0, flat_band=False)
    c["equal_th_131x97"] = sf.make_frame(11, 131, 97, 2, ini_th=9, min_th=9)
    c["extreme_th_150x110"] = sf.make_frame(13, 150, 110, 1, ini_th=255, min_th=1)
    c["uniform_67"] = sf.uniform_frame()
    c["four_corners_67"] = sf.four_corner_frame()
    # the levels of the geometry table as single-level pyramids: one cell, no cell (66 wide, 66 high), a clipped and a removed last
    # cell, and its twin
    c["geom_67x67"] = sf.make_frame(17, 67, 67, 1, weak_band=False, flat_band=False, density=3.0)
    c["geom_66x67"] = sf.make_frame(19, 66, 67, 1, weak_band=False, flat_band=False)
    c["geom_67x66"] = sf.make_frame(37, 67, 66, 1, weak_band=False, flat_band=False)
    c["geom_2133x67"] = sf.make_frame(23, 2133, 67, 1, density=2.0)
    c["geom_67x2133"] = sf.make_frame(29, 67, 2133, 1, density=2.0, weak_band=False, flat_band=False)
    c["vga_640x480_L8"] = sf.make_frame(41, 640, 480, 8)
    return c


CASE_NAMES = ("mix_160x120", "mix_240x180_low_th", "dense_200x150", "equal_th_131x97", "extreme_th_150x110", "uniform_67",
              "four_corners_67", "geom_67x67", "geom_66x67", "geom_67x66", "geom_2133x67", "geom_67x2133", "vga_640x480_L8")


@functools.lru_cache(maxsize=None)
def case(name):
    """(frame, expected detect, keypoints for IC_Angle as (xy, level), expected IC_Angle) of a committed case, computed once."""
    if name == "vga_752x480_L8":
        frame = sf.make_frame(31, 752, 480, 8)
    elif name.startswith("levels_"):
        frame = sf.make_frame(40 + int(name[7:]), 160, 120, int(name[7:]))
    else:
        frame = _cases()[name]
    exp = detect(frame)
    kxy, klevel = keypoints_of(frame, exp)
    return frame, exp, (kxy, klevel), ic_angle(frame.pyramid, kxy, klevel)


def keypoints_of(frame, exp):
    """The keypoints ComputeKeyPointsOctTree would hand to computeOrientation if the octree kept every candidate once: the distinct
    corners with minBorder added."""
    if len(exp["level"]) == 0:
        return np.zeros((0, 2), F), np.zeros(0, np.int32)
    rows = np.unique(np.concatenate([exp["level"][:, None].astype(F), exp["xy"]], 1), axis=0)
    return np.ascontiguousarray(rows[:, 1:] + F(16)), rows[:, 0].astype(np.int32)


def assert_detect_same(got, exp, what=""):
    for k in ("level_count", "xy", "response", "level", "cell", "used_min_th"):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, f"{what}: {k} shape {g.shape} != {e.shape}"
        if g.dtype == np.float32:
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(g, e), f"{what}: {k} differs at {np.argwhere(g != e)[:5].tolist()}"


def assert_angles_same(got, exp, what=""):
    for k in ("m10", "m01"):
        assert np.array_equal(got[k], exp[k]), f"{what}: {k} differs at {np.nonzero(got[k] != exp[k])[0][:5].tolist()}"
    g, e = got["angle"].view(np.uint32), exp["angle"].view(np.uint32)
    assert np.array_equal(g, e), f"{what}: angle differs at {np.nonzero(g != e)[0][:5].tolist()}: {got['angle'][g != e][:5]} != {exp['angle'][g != e][:5]}"
