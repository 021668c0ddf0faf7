"""The search of ORBmatcher::Fuse (src/ORBmatcher.cc:1148-1338 and :1340-1455) for one (keyframe, map point) pair, restated in
numpy from the reference's statements: explicit float32 scalars, every operation rounded once and none fused, Eigen's three-term
reductions as a0 + (a1 + a2), sqrt / atan2 / cos / sin / log as the FP64 function rounded once, the keyframe's grid as lists of
lists filled the way KeyFrame's constructor copies Frame::AssignFeaturesToGrid (src/Frame.cc:397-417, 726-736), and the walk of
KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:704-745) over those lists.  The expected values of tests/test_fuse_cpu.py and
tests/test_gpu_fuse.py; written without reading csrc/orb_fuse.h."""
import functools
import math

import numpy as np

from orb_slam3_study_kr_amd import synth_fuse as sf

F = np.float32
SKIPPED, BEHIND, OUTSIDE, DISTANCE, ANGLE, EMPTY, SEARCHED = range(7)
CHI2, SIM3 = 0, 1
NAMES = sf.NAMES
INT_MIN = -2 ** 31


def c_int(x):
    """(int)x of a float as the reference's build converts it (cvttss2si): truncation, INT_MIN for NaN and for what no int holds."""
    x = float(x)
    if math.isnan(x) or x >= 2.0 ** 31 or x < -2.0 ** 31:
        return INT_MIN
    return int(x)


def c_round(x):
    """std::round of a float: half away from zero (exact in float64)."""
    x = float(x)
    return math.copysign(math.floor(abs(x) + 0.5), x)


def sum3(a0, a1, a2):
    return F(a0 + F(a1 + a2))


def sqrt_rn(x):
    return F(np.sqrt(np.float64(x)))


def grid_of(t):
    """mGrid[ix][iy]: the keypoint indices of every cell in keypoint order."""
    grid = [[[] for _ in range(t.rows)] for _ in range(t.cols)]
    gx, gy = F(t.grid_min[0]), F(t.grid_min[1])
    winv, hinv = F(t.cell_inv[0]), F(t.cell_inv[1])
    for i in range(t.n_keys):
        px = c_int(c_round(F(F(t.key_xy[i, 0] - gx) * winv)))
        py = c_int(c_round(F(F(t.key_xy[i, 1] - gy) * hinv)))
        if px < 0 or px >= t.cols or py < 0 or py >= t.rows:
            continue
        grid[px][py].append(i)
    return grid


def project(t, pc):
    if t.camera == sf.KB8:   # src/CameraModels/KannalaBrandt8.cpp:67-84
        k = [F(x) for x in t.kb8]
        x2y2 = F(F(pc[0] * pc[0]) + F(pc[1] * pc[1]))
        theta = F(np.arctan2(np.float64(sqrt_rn(x2y2)), np.float64(pc[2])))
        psi = F(np.arctan2(np.float64(pc[1]), np.float64(pc[0])))
        t2 = F(theta * theta)
        t3 = F(theta * t2)
        t5 = F(t3 * t2)
        t7 = F(t5 * t2)
        t9 = F(t7 * t2)
        r = F(F(F(F(theta + F(k[0] * t3)) + F(k[1] * t5)) + F(k[2] * t7)) + F(k[3] * t9))
        u = F(F(F(F(t.fx) * r) * F(np.cos(np.float64(psi)))) + F(t.cx))
        v = F(F(F(F(t.fy) * r) * F(np.sin(np.float64(psi)))) + F(t.cy))
        return u, v
    # src/CameraModels/Pinhole.cpp:43-49
    return F(F(F(F(t.fx) * pc[0]) / pc[2]) + F(t.cx)), F(F(F(F(t.fy) * pc[1]) / pc[2]) + F(t.cy))


def features_in_area(t, grid, x, y, r):
    """KeyFrame::GetFeaturesInArea: the indices in the order of its loops."""
    out = []
    gx, gy = F(t.grid_min[0]), F(t.grid_min[1])
    winv, hinv = F(t.cell_inv[0]), F(t.cell_inv[1])
    min_cx = max(0, c_int(np.floor(F(F(F(x - gx) - r) * winv))))
    if min_cx >= t.cols:
        return out
    max_cx = min(t.cols - 1, c_int(np.ceil(F(F(F(x - gx) + r) * winv))))
    if max_cx < 0:
        return out
    min_cy = max(0, c_int(np.floor(F(F(F(y - gy) - r) * hinv))))
    if min_cy >= t.rows:
        return out
    max_cy = min(t.rows - 1, c_int(np.ceil(F(F(F(y - gy) + r) * hinv))))
    if max_cy < 0:
        return out
    for ix in range(min_cx, max_cx + 1):
        for iy in range(min_cy, max_cy + 1):
            for j in grid[ix][iy]:
                dx = F(t.key_xy[j, 0] - x)
                dy = F(t.key_xy[j, 1] - y)
                if abs(dx) < r and abs(dy) < r:
                    out.append(j)
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def pair(t, tables, grid, pts, p, mode):
    """One (target, point) pair: the nine outputs as a tuple in the order of NAMES."""
    sfac, inv_sigma2, log_sf = tables
    none = (F(0), F(0), F(0), -1, F(0), 0, -1, 256)
    if pts.skip is not None and pts.skip[p]:
        return (SKIPPED,) + none
    P = [F(x) for x in pts.pos[p]]
    R = np.asarray(t.Rcw, F).reshape(3, 3)
    pc = [F(sum3(F(R[r, 0] * P[0]), F(R[r, 1] * P[1]), F(R[r, 2] * P[2])) + F(t.tcw[r])) for r in range(3)]
    if pc[2] < F(0):
        return (BEHIND,) + none
    invz = F(F(1) / pc[2])
    u, v = project(t, pc)
    min_x, max_x, min_y, max_y = [F(b) for b in t.bounds]
    if not (u >= min_x and u < max_x and v >= min_y and v < max_y):
        return (OUTSIDE,) + none
    ur = F(u - F(F(t.bf) * invz))
    PO = [F(P[k] - F(t.Ow[k])) for k in range(3)]
    dist = sqrt_rn(sum3(F(PO[0] * PO[0]), F(PO[1] * PO[1]), F(PO[2] * PO[2])))
    if dist < F(F(0.8) * pts.min_dist[p]) or dist > F(F(1.2) * pts.max_dist[p]):
        return (DISTANCE, u, v, ur, -1, F(0), 0, -1, 256)
    Pn = [F(x) for x in pts.normal[p]]
    if np.float64(sum3(F(PO[0] * Pn[0]), F(PO[1] * Pn[1]), F(PO[2] * Pn[2]))) < 0.5 * np.float64(dist):
        return (ANGLE, u, v, ur, -1, F(0), 0, -1, 256)
    # MapPoint::PredictScale (src/MapPoint.cc:531-546)
    ratio = F(pts.max_dist[p] / dist)
    n_scale = c_int(np.ceil(F(F(np.log(np.float64(ratio))) / log_sf)))
    level = 0 if n_scale < 0 else min(n_scale, t.n_levels - 1)
    radius = F(F(t.th) * sfac[level])
    indices = features_in_area(t, grid, u, v, radius)
    if not indices:
        return (EMPTY, u, v, ur, level, radius, 0, -1, 256)
    d_point = pts.desc[p]
    best_dist, best_idx, n_cand = 256, -1, 0
    for j in indices:
        octave = int(t.key_octave[j])
        if octave < level - 1 or octave > level:
            continue
        if mode == CHI2:
            ex = F(u - t.key_xy[j, 0])
            ey = F(v - t.key_xy[j, 1])
            if t.key_uright is not None and t.key_uright[j] >= 0:
                er = F(ur - t.key_uright[j])
                e2 = F(F(F(ex * ex) + F(ey * ey)) + F(er * er))
                if np.float64(F(e2 * inv_sigma2[octave])) > 7.8:
                    continue
            else:
                e2 = F(F(ex * ex) + F(ey * ey))
                if np.float64(F(e2 * inv_sigma2[octave])) > 5.99:
                    continue
        n_cand += 1
        d = hamming(d_point, t.desc[j])
        if d < best_dist:
            best_dist, best_idx = d, j
    return (SEARCHED, u, v, ur, level, radius, n_cand, best_idx, best_dist)


def search(targets, pts, mode):
    """Every pair of the call: the dict of OrbMatcher.fuse_search."""
    K, n = len(targets), pts.n
    out = {name: np.zeros((K, n), np.float32 if name in ("u", "v", "ur", "radius") else np.int32) for name in NAMES}
    with np.errstate(all="ignore"):
        for k, t in enumerate(targets):
            tables, grid = t.level_tables(), grid_of(t)
            for p in range(n):
                for name, value in zip(NAMES, pair(t, tables, grid, pts, p, mode)):
                    out[name][k, p] = value
    return out


same_bits = sf.same_bits   # the names of the outputs that differ in any bit


# ---- the cases both test files run, each with its restatement computed once

CAMERAS = {"mono": dict(camera=sf.PINHOLE, stereo=False), "stereo": dict(camera=sf.PINHOLE, stereo=True), "kb8": dict(camera=sf.KB8, stereo=False)}


@functools.lru_cache(maxsize=None)
def shape_case(camera: str, mode: int):
    """K = 8 targets, P = 300: keypoints per target 200, 0, 1, 200, ...; target 1 has no keypoint, target 3 looks away (no point
    passes), target 4 has th = 40 (a window of more than 64 cells), target 5 has 70 keypoints on one spot (a cell of more than 64
    entries), target 6 has OSH_FUSE_MAX_CELL_ENTRIES = 255 of them; every 17th point is a null entry."""
    targets, pts = sf.make_case(11, 8, 300, [200, 0, 1, 200, 200, 200, 300, 200], skip_every=17, away=(3,), cluster={5: 70, 6: 255}, **CAMERAS[camera])
    targets[4].th = 40.0
    return targets, pts, search(targets, pts, mode)


def head(targets, pts, exp, K, P):
    """The first K targets and the first P points of a case, with the matching part of its expected outputs."""
    sub = sf.Points(pts.pos[:P], pts.normal[:P], pts.min_dist[:P], pts.max_dist[:P], pts.desc[:P], None if pts.skip is None else pts.skip[:P])
    return targets[:K], sub, {name: np.ascontiguousarray(exp[name][:K, :P]) for name in NAMES}


def bits(value, n):
    """A 32-byte descriptor whose first n bits are those of the zero descriptor flipped, on top of `value` in every byte."""
    d = np.full(32, value, np.uint8)
    for b in range(n):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


@functools.lru_cache(maxsize=None)
def constructed_case():
    """One pinhole target at the origin with the identity pose, fx = fy = 256, cx = 320, cy = 240, bounds [0, 640) x [0, 480), 10-pixel
    cells and scale factor 1.2, and points built so that a gate's two sides meet exactly.  Returns targets, points, the stage each
    point must get by the reference's arithmetic (worked out in the comments, not taken from any run) and the names of the points."""
    t = sf.Target(Rcw=np.eye(3, dtype=F), tcw=np.zeros(3, F), Ow=np.zeros(3, F), th=3.0)
    sfac = t.level_tables()[0]
    rows = []   # name, pos, normal, min_dist, max_dist, skip, stage

    def add(name, pos, stage, normal=None, min_dist=0.1, max_dist=None, skip=0):
        # max_dist defaults to the distance as the reference computes it: ratio 1, log 0, level 0, radius 3
        pos = np.asarray(pos, F)
        with np.errstate(all="ignore"):
            d = sqrt_rn(sum3(F(pos[0] * pos[0]), F(pos[1] * pos[1]), F(pos[2] * pos[2])))
        rows.append((name, pos, np.asarray(normal if normal is not None else [0, 0, 1], F), F(min_dist), F(max_dist if max_dist is not None else d), skip, stage))

    keys, octs, descs = [], [], []

    def key(x, y, octave, desc):
        keys.append((x, y)); octs.append(octave); descs.append(desc)
        return len(keys) - 1

    # z exactly 0 is not "< 0": it goes on and x / 0 = inf (or 0 / 0 = NaN) fails IsInImage.  -0.0 < 0 is false as well.
    add("z_zero", [0.5, 0.25, 0.0], OUTSIDE)
    add("z_zero_centre", [0.0, 0.0, 0.0], OUTSIDE)
    add("z_minus_zero", [0.5, 0.25, -0.0], OUTSIDE)
    add("z_negative", [0.5, 0.25, -1e-30], BEHIND)
    # u = 256 * x / 2 + 320: x = -2.5 gives exactly 0 = mnMinX (inside), x = 2.5 exactly 640 = mnMaxX (outside).  On the axis the
    # normal (0, 0, 1) gives PO.Pn = 2 against 0.5 * dist = 1.6: the angle gate passes; nothing is near: an empty window
    add("u_min", [-2.5, 0.0, 2.0], EMPTY)
    add("u_max", [2.5, 0.0, 2.0], OUTSIDE)
    add("v_min", [0.0, -1.875, 2.0], EMPTY)      # v = 256 * -1.875 / 2 + 240 = 0
    add("v_max", [0.0, 1.875, 2.0], OUTSIDE)     # 480
    # dist = 4 exactly.  0.8f * 5 = 4.0000000596 rounds to 4: dist < 4 is false, the gate passes.  1.2f * 3.3333333 is below or at 4
    # only by rounding, so the upper end uses max_dist = 2.5 with dist = 3: 1.2f * 2.5 = 3.0000001192 rounds to 3, dist > 3 is false
    add("dist_at_min", [0.0, 0.0, 4.0], EMPTY, min_dist=5.0, max_dist=8.0)
    add("dist_below_min", [0.0, 0.0, np.nextafter(F(4.0), F(0.0))], DISTANCE, min_dist=5.0, max_dist=8.0)
    add("dist_at_max", [0.0, 0.0, 3.0], EMPTY, min_dist=0.1, max_dist=2.5)
    add("dist_above_max", [0.0, 0.0, np.nextafter(F(3.0), F(4.0))], DISTANCE, min_dist=0.1, max_dist=2.5)
    # PO = (0, 0, 4), Pn = (0, 0, 0.5): PO.Pn = 2 = 0.5 * dist exactly, not below: passes.  One ulp less fails
    add("angle_at_half", [0.0, 0.0, 4.0], EMPTY, normal=[0, 0, 0.5], max_dist=4.0)
    add("angle_below_half", [0.0, 0.0, 4.0], ANGLE, normal=[0, 0, np.nextafter(F(0.5), F(0.0))], max_dist=4.0)
    # ratio = max_dist / dist exactly scaleFactor^k as the level table holds it: whatever the rounded log gives, all three agree
    for k in (1, 3):
        add(f"ratio_sf^{k}", [0.0, 0.0, 2.0], EMPTY, max_dist=F(F(2.0) * sfac[k]))
    # level 0 (max_dist = dist: log 1 = 0) with keypoints at octaves 0 and 1 at the projection (320, 240): the band [-1, 0] keeps
    # octave 0 only; the last level (a huge ratio is clamped) with octaves 6 and 7 kept, 5 not
    d0 = np.zeros(32, np.uint8)
    add("level_0", [0.5, 0.5, 2.0], SEARCHED)                               # u = 384, v = 304
    k_l0 = key(384.5, 304.5, 0, bits(0, 9)); key(384.25, 304.25, 1, bits(0, 1))
    add("level_top", [1.0, 0.0, 2.0], SEARCHED, max_dist=1000.0)            # u = 448, v = 240, radius = 3 * 1.2^7 = 10.7
    k_top = key(449.0, 241.0, 6, bits(0, 5)); key(447.0, 239.0, 7, bits(0, 7)); key(448.0, 240.0, 5, bits(0, 0))
    # windows clipped at each edge of the grid (64 x 48 cells of 10 pixels over the image), a keypoint inside each
    add("clip_left", [-2.49, -0.5, 2.0], SEARCHED)                          # u = 1.28, v = 176
    key(1.0, 176.0, 0, d0)
    # PosInGrid rounds: x = 634.9 is the last that lands in column 63 (635 would be column 64, in no cell)
    add("clip_right", [2.4765625, -0.5, 2.0], SEARCHED)                     # u = 637: ceil(64.0) = 64 is cut to column 63
    key(634.9, 176.0, 0, d0)
    add("clip_top", [-0.5, -1.87, 2.0], SEARCHED)                           # u = 256, v = 0.64
    key(256.0, 1.0, 0, d0)
    add("clip_bottom", [-0.5, 1.8515625, 2.0], SEARCHED)                    # v = 477: row 48 is cut to 47
    key(256.0, 474.9, 0, d0)
    # keypoints in the window's cells, none within the radius 3 of (192, 112): empty
    add("cell_not_radius", [-1.0, -1.0, 2.0], EMPTY)
    key(196.0, 112.0, 0, d0); key(192.0, 116.0, 0, d0); key(188.0, 108.0, 0, d0)
    # equal distances: (64, 368) has two keypoints at distance 3 in different cells (x 62.0 -> column 6, x 65.5 -> column 7: the
    # lower column is scanned first, though it comes later in the keypoint order); (576, 368) has two in one cell: keypoint order
    add("tie_cells", [-2.0, 1.0, 2.0], SEARCHED)
    k_tie_late = key(65.5, 368.0, 0, bits(0, 3)); k_tie_first = key(62.0, 368.0, 0, bits(255, 253))
    add("tie_one_cell", [2.0, 1.0, 2.0], SEARCHED)
    k_tie_a = key(576.5, 368.5, 0, bits(0, 4)); key(577.0, 369.0, 0, bits(255, 252))
    add("skipped", [0.0, 0.0, 2.0], SKIPPED, skip=1)
    add("nan_position", [np.nan, 0.0, 2.0], OUTSIDE)
    add("inf_max_dist", [0.5, 0.5, 2.0], SEARCHED, max_dist=np.inf)         # ratio inf: no int holds ceil(inf): level 0, as level_0

    t.key_xy = np.asarray(keys, F)
    t.key_octave = np.asarray(octs, np.int32)
    t.desc = np.stack(descs)
    n = len(rows)
    pts = sf.Points(np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.asarray([r[3] for r in rows], F), np.asarray([r[4] for r in rows], F),
                    np.zeros((n, 32), np.uint8), np.asarray([r[5] for r in rows], np.uint8))
    names = [r[0] for r in rows]
    stages = np.asarray([r[6] for r in rows], np.int32)
    best = {"level_0": k_l0, "level_top": k_top, "tie_cells": k_tie_first, "tie_one_cell": k_tie_a, "inf_max_dist": k_l0}
    # an off-grid window needs a grid smaller than the image: a second target whose grid covers x >= 400 only sees level_0's window
    # (u = 384) end left of its first column: ceil((384 - 400 + 3) / 10) = -1 < 0: an early return, an empty window
    t2 = sf.Target(Rcw=np.eye(3, dtype=F), tcw=np.zeros(3, F), Ow=np.zeros(3, F), th=3.0, grid_min=(400.0, 0.0), cols=24, rows=48,
                   key_xy=t.key_xy, key_octave=t.key_octave, desc=t.desc)
    # a radius no int holds a cell number for (th = 3e38): (int)ceil(...) is INT_MIN in the reference's build, so nMaxCellX < 0 and
    # GetFeaturesInArea returns early: every pair that reaches the window is EMPTY there
    t3 = sf.Target(Rcw=np.eye(3, dtype=F), tcw=np.zeros(3, F), Ow=np.zeros(3, F), th=3.0e38, key_xy=t.key_xy, key_octave=t.key_octave, desc=t.desc)
    return [t, t2, t3], pts, stages, names, best
