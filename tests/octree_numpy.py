"""ORBextractor::DistributeOctTree (reference src/ORBextractor.cc:480-779) restated from the definition in include/orbslam3_hip.h
as the ordered list it describes: nodes are objects, the list is a Python list whose index 0 is the front, a division pushes its
non-empty children to the front and erases the node.  Nothing here is shared with csrc/orb_octree.h, which works on arrays and
prefix sums; tests/test_octree_cpu.py pins the two to each other bit for bit.

distribute() also takes a census of what a list exercised, for the census test.  cases() are the committed lists."""
import functools
import math

import numpy as np

F = np.float32


def c_round(v) -> int:
    """C round() of a float32: to nearest, halves away from zero."""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def half(d: int) -> int:
    """ceil((float)d / 2) of a box extent d >= 0."""
    return int(math.ceil(float(F(d) / F(2))))


class Node:
    __slots__ = ("ulx", "urx", "uly", "bry", "keys")

    def __init__(self, ulx, urx, uly, bry):
        self.ulx, self.urx, self.uly, self.bry, self.keys = ulx, urx, uly, bry, []


def divide(node, xy, cs):
    """The four children n1 left-top, n2 right-top, n3 left-bottom, n4 right-bottom; a key goes left when x < (float)mx and top
    when y < (float)my, whatever its box."""
    mx, my = node.ulx + half(node.urx - node.ulx), node.uly + half(node.bry - node.uly)
    ch = [Node(node.ulx, mx, node.uly, my), Node(mx, node.urx, node.uly, my), Node(node.ulx, mx, my, node.bry), Node(mx, node.urx, my, node.bry)]
    for k in node.keys:
        x, y = xy[k]
        cs["beyond_right"] += int(x >= F(node.urx))
        ch[(0 if x < F(mx) else 1) + (0 if y < F(my) else 2)].keys.append(k)
    return ch


def new_census():
    return dict(n_ini=0, ratio_half=False, n_ini_zero=False, root_clamped=0, finish="", multi_left=False, rounds_a=0, rounds_b=0,
                b_break=False, sort_sizes=[], sort_tied_over_16=False, response_tie=0, beyond_right=0, count=0)


def distribute(xy, response, W, H, N):
    """(kept input indices in result order, census) of one list: n candidates xy [n, 2] relative to (minX, minY) and response [n],
    the area W = maxX - minX by H = maxY - minY, N features wanted."""
    xy = np.ascontiguousarray(xy, F).reshape(-1, 2)
    response = np.ascontiguousarray(response, F).reshape(-1)
    cs = new_census()
    ratio = F(W) / F(H)
    n_ini = c_round(ratio)
    cs["ratio_half"] = float(ratio) * 2 == math.floor(float(ratio) * 2) and float(ratio) != math.floor(float(ratio))
    if n_ini == 0:      # intended deviation: the reference divides by zero
        n_ini, cs["n_ini_zero"] = 1, True
    cs["n_ini"] = n_ini
    hx = F(W) / F(n_ini)
    roots = [Node(int(F(hx * F(i))), int(F(hx * F(i + 1))), 0, H) for i in range(n_ini)]
    for k in range(len(xy)):
        r = int(F(xy[k, 0] / hx))
        if r >= n_ini:  # intended deviation: the reference indexes past its vector
            r, cs["root_clamped"] = n_ini - 1, cs["root_clamped"] + 1
        roots[r].keys.append(k)
    nodes = [r for r in roots if r.keys]

    finish = False
    while not finish:                                   # round A
        prev = len(nodes)
        cs["rounds_a"] += 1
        created, E, stay = [], [], []
        for node in nodes:                              # front to back; what is pushed to the front is not visited
            if len(node.keys) == 1:
                stay.append(node)
                continue
            for c in divide(node, xy, cs):
                if c.keys:
                    created.append(c)
                    if len(c.keys) > 1:
                        E.append(c)
        nodes = created[::-1] + stay
        if len(nodes) >= N or len(nodes) == prev:
            finish = True
            cs["finish"] = "A_size" if len(nodes) >= N else "A_prev"
        elif len(nodes) + 3 * len(E) > N:
            while not finish:                           # round B
                prev = len(nodes)
                cs["rounds_b"] += 1
                e_prev, E = E, []
                keys = [(len(e.keys), e.ulx) for e in e_prev]
                order = sorted(range(len(e_prev)), key=lambda j: keys[j])      # stable: intended deviation from std::sort
                cs["sort_sizes"].append(len(e_prev))
                if len(e_prev) > 16 and len(set(keys)) < len(keys):
                    cs["sort_tied_over_16"] = True
                for at, j in enumerate(reversed(order)):
                    node = e_prev[j]
                    for c in divide(node, xy, cs):
                        if c.keys:
                            nodes.insert(0, c)
                            if len(c.keys) > 1:
                                E.append(c)
                    nodes.remove(node)                  # by identity: Node defines no __eq__
                    if len(nodes) >= N:
                        cs["b_break"] = cs["b_break"] or at + 1 < len(order)
                        break
                if len(nodes) >= N or len(nodes) == prev:
                    finish = True
                    cs["finish"] = "B_size" if len(nodes) >= N else "B_prev"
    cs["multi_left"] = any(len(nd.keys) > 1 for nd in nodes)
    kept = []
    for nd in nodes:
        best = nd.keys[0]
        for k in nd.keys[1:]:
            if response[k] > response[best]:
                best = k
        cs["response_tie"] += int(sum(1 for k in nd.keys if response[k] == response[best]) > 1)
        kept.append(best)
    cs["count"] = len(kept)
    return np.asarray(kept, np.int32), cs


def features_per_level(nfeatures, scale_factor, nlevels):
    """mnFeaturesPerLevel as the stand-in's constructor leaves it (csrc/hosttest/orbextractor.cc): a geometric series in float32
    steps, each term rounded half to even, the last level taking what is left."""
    q = F(1.0) / F(scale_factor)
    share = F(F(nfeatures) * F(F(1) - q) / F(F(1) - F(float(q) ** nlevels)))
    out, given = [], 0
    for _ in range(nlevels - 1):
        out.append(int(np.rint(share)))
        given += out[-1]
        share = F(share * q)
    return out + [max(nfeatures - given, 0)]


def _grid_points(rng, n, W, H, max_response=40, integer=True):
    x = rng.integers(0, W, n).astype(F) if integer else (rng.random(n) * W).astype(F)
    y = rng.integers(0, H, n).astype(F) if integer else (rng.random(n) * H).astype(F)
    x = np.minimum(x, np.nextafter(F(W), F(0)))
    return np.stack([x, y], 1), rng.integers(1, max_response + 1, n).astype(F)


def _clustered(rng, n, W, H, n_clusters, spread):
    c = np.stack([rng.integers(0, W, n_clusters), rng.integers(0, H, n_clusters)], 1)
    p = c[rng.integers(0, n_clusters, n)] + np.rint(rng.normal(0, spread, (n, 2)))
    p[:, 0] = np.clip(p[:, 0], 0, W - 1)
    p[:, 1] = np.clip(p[:, 1], 0, H - 1)
    return p.astype(F), rng.integers(1, 30, n).astype(F)


# ---- the committed lists: name -> (xy, response, W, H, N).  Seeds were adjusted on the CPU until the census of
# tests/test_octree_cpu.py held.
@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    rng = np.random.default_rng(20261)
    z2, z1 = np.zeros((0, 2), F), np.zeros(0, F)
    c["empty_128x88"] = (z2, z1, 128, 88, 10)
    c["single_128x88"] = (np.array([[5, 7]], F), np.array([3], F), 128, 88, 10)
    c["n0_features_128x88"] = _grid_points(rng, 60, 128, 88) + (128, 88, 0)
    c["n1_features_128x88"] = _grid_points(rng, 60, 128, 88) + (128, 88, 1)
    c["negative_features_128x88"] = _grid_points(rng, 60, 128, 88) + (128, 88, -5)
    c["more_features_than_keys_128x88"] = _grid_points(rng, 40, 128, 88) + (128, 88, 100)
    c["grid_500_128x88"] = _grid_points(rng, 500, 128, 88) + (128, 88, 120)
    c["grid_130_128x88_n65"] = _grid_points(rng, 130, 128, 88) + (128, 88, 65)
    c["wide_300x100"] = _grid_points(rng, 400, 300, 100) + (300, 100, 90)
    c["wide_200x100"] = _grid_points(rng, 257, 200, 100) + (200, 100, 64)
    c["half_ratio_150x100"] = _grid_points(rng, 300, 150, 100) + (150, 100, 77)
    c["portrait_40x100"] = _grid_points(rng, 200, 40, 100) + (40, 100, 50)
    c["fractional_300x100"] = _grid_points(rng, 333, 300, 100, integer=False) + (300, 100, 101)
    c["thirds_100x30"] = _grid_points(rng, 150, 100, 30) + (100, 30, 40)
    # a lone root whose keys all fall into one quadrant: the list does not grow and one keypoint is kept
    c["lone_quadrant_128x88"] = (np.array([[3, 2], [10, 20], [40, 30], [63, 43]], F), np.array([5, 9, 9, 1], F), 128, 88, 10)
    # two candidates on one pixel, beside others: that node is divided until the list stops growing
    c["same_pixel_128x88"] = (np.array([[70, 50], [70, 50], [10, 10], [100, 80], [20, 70]], F), np.array([4, 4, 2, 8, 1], F), 128, 88, 20)
    c["only_same_pixel_128x88"] = (np.array([[70, 50], [70, 50]], F), np.array([4, 6], F), 128, 88, 20)
    # rows below the area are legal: y is only compared
    xy, resp = _grid_points(rng, 120, 150, 100)
    xy[::7, 1] += F(100)
    c["below_area_150x100"] = (xy, resp, 150, 100, 60)
    c["clusters_300x100"] = _clustered(rng, 450, 300, 100, 9, 4.0) + (300, 100, 150)
    c["clusters_128x88_tight"] = _clustered(rng, 380, 128, 88, 5, 1.5) + (128, 88, 200)
    c["one_row_60x1"] = (np.stack([np.arange(0, 60, dtype=F) // 2 * 2, np.zeros(60, F)], 1), (np.arange(60) % 7 + 1).astype(F), 60, 1, 45)
    # the last representable x below the width: its root index is taken as nIni - 1 when the division rounds up to nIni
    c["right_edge_100x30"] = (np.array([[np.nextafter(F(100), F(0)), 5], [99, 3], [50, 2], [0, 29]], F), np.array([1, 2, 3, 4], F), 100, 30, 8)
    c["level_720x448"] = _grid_points(rng, 3000, 720, 448, max_response=120) + (720, 448, 217)
    return c


CASE_NAMES = ("empty_128x88", "single_128x88", "n0_features_128x88", "n1_features_128x88", "negative_features_128x88",
              "more_features_than_keys_128x88", "grid_500_128x88", "grid_130_128x88_n65", "wide_300x100", "wide_200x100",
              "half_ratio_150x100", "portrait_40x100", "fractional_300x100", "thirds_100x30", "lone_quadrant_128x88", "same_pixel_128x88",
              "only_same_pixel_128x88", "below_area_150x100", "clusters_300x100", "clusters_128x88_tight", "one_row_60x1", "right_edge_100x30", "level_720x448")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(kept, census) of a committed list, computed once and shared by the tests; treat as read-only."""
    xy, resp, W, H, N = cases()[name]
    return distribute(xy, resp, W, H, N)


def fast_lists(fast_case, nfeatures=1000, scale_factor=1.2):
    """The lists ComputeKeyPointsOctTree hands to DistributeOctTree for a committed FAST case (tests/fast_numpy.case): per level the
    candidates relative to minBorder, the detect area and mnFeaturesPerLevel[level]."""
    frame, exp = fast_case[0], fast_case[1]
    per_level = features_per_level(nfeatures, scale_factor, len(frame.pyramid))
    lists = []
    for l, im in enumerate(frame.pyramid):
        sel = exp["level"] == l
        W, H = im.shape[1] - 32, im.shape[0] - 32
        if W <= 0 or H <= 0:
            continue
        lists.append((np.ascontiguousarray(exp["xy"][sel]), np.ascontiguousarray(exp["response"][sel]), W, H, per_level[l]))
    return lists
