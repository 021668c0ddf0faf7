"""ORBextractor::ComputePyramid as include/orbslam3_hip.h defines it, restated in numpy: the level sizes, the tap tables by array
arithmetic in float64 / float32 with np.rint, the pixel formula in int64, and the border by np.pad(mode="reflect") where the level is
larger than the border and by the closed form of reflect-101 otherwise.  It shares no code with csrc/orb_pyramid.h.  case(name)
yields the committed cases: seeded images, their inv_scale and border, and the expected bordered levels."""
import functools

import numpy as np

F = np.float32
Q = F(1) / F(1.2)
CHAIN = (F(1), F(1 / 1.2), F(1 / 1.44), F(1 / 1.728))


def cv_round(x) -> int:
    return int(np.rint(F(x)))


def level_shapes(rows, cols, inv_scale):
    return [(cv_round(F(rows) * F(s)), cv_round(F(cols) * F(s))) for s in inv_scale]


def axis_table(src: int, dst: int, rows: bool):
    """s0, s1 (int64), w0, w1 (int64) and the float32 fraction of every destination index of one axis."""
    scale = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F)).astype(F)
    hit = {}
    if rows:
        hit["low"], hit["high"] = int((s < 0).sum()), int((s + 1 > src - 1).sum())
        s0, s1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    else:
        low = s < 0
        s[low], f[low] = 0, 0
        high = s >= src - 1
        s[high], f[high] = src - 1, 0
        hit["low"], hit["high"] = int(low.sum()), int(high.sum())
        s0, s1 = s, np.minimum(s + 1, src - 1)
    a = (F(1) - f) * F(2048)
    b = f * F(2048)
    w0, w1 = np.rint(a).astype(np.int64), np.rint(b).astype(np.int64)
    hit["ties"] = int((np.abs(a - np.floor(a) - F(0.5)) == 0).sum() + (np.abs(b - np.floor(b) - F(0.5)) == 0).sum())
    hit["full"] = int(((w0 == 2048) & (w1 == 0)).sum())
    hit["sum_off"] = int((w0 + w1 != 2048).sum())
    return s0, s1, w0, w1, hit


def is_halving(src_shape, dst_shape) -> bool:
    return src_shape[1] == 2 * dst_shape[1] and src_shape[0] == 2 * dst_shape[0]


def resample(S: np.ndarray, rows: int, cols: int, census=None) -> np.ndarray:
    S = S.astype(np.int64)
    if is_halving(S.shape, (rows, cols)):
        if census is not None:
            census["halving"] = census.get("halving", 0) + 1
        return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1, hx = axis_table(S.shape[1], cols, False)
    y0, y1, b0, b1, hy = axis_table(S.shape[0], rows, True)
    if census is not None:
        for axis, h in (("col", hx), ("row", hy)):
            for k, v in h.items():
                census[f"{axis}_{k}"] = census.get(f"{axis}_{k}", 0) + v
    h = S[:, x0] * a0[None, :] + S[:, x1] * a1[None, :]
    out = ((((b0[:, None] * (h[y0] >> 4)) >> 16) + ((b1[:, None] * (h[y1] >> 4)) >> 16) + 2) >> 2)
    return (out & 0xFF).astype(np.uint8)


def reflect_index(p: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    m = np.mod(p, period)
    return np.where(m < n, m, period - m)


def bordered(level: np.ndarray, border: int) -> np.ndarray:
    rows, cols = level.shape
    if border == 0:
        return level.copy()
    if rows > border and cols > border:
        return np.pad(level, border, mode="reflect")
    ys = reflect_index(np.arange(-border, rows + border), rows)
    xs = reflect_index(np.arange(-border, cols + border), cols)
    return level[ys][:, xs]


def build(image: np.ndarray, inv_scale, border: int = 19, census=None):
    """The levels and the bordered levels of one image."""
    shapes = level_shapes(image.shape[0], image.shape[1], inv_scale)
    assert shapes[0] == image.shape
    levels = [np.ascontiguousarray(image)]
    for r, c in shapes[1:]:
        levels.append(resample(levels[-1], r, c, census))
    if census is not None:
        for lv in levels:
            census["one_row"] = census.get("one_row", 0) + (lv.shape[0] == 1)
            census["one_col"] = census.get("one_col", 0) + (lv.shape[1] == 1)
            census["len_1_reflected"] = census.get("len_1_reflected", 0) + (border > 0 and 1 in lv.shape)
            census["len_le_border"] = census.get("len_le_border", 0) + (min(lv.shape) <= border)
    return levels, [bordered(lv, border) for lv in levels]


def image(seed: int, rows: int, cols: int, kind: str = "noise") -> np.ndarray:
    if kind == "zeros":
        return np.zeros((rows, cols), np.uint8)
    if kind == "ones":
        return np.full((rows, cols), 255, np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:rows, 0:cols]
        return (((x + y) & 1) * 255).astype(np.uint8)
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (rows, cols)).astype(np.float64)
    if kind == "smooth":   # blobs over a ramp: corners for the detector
        y, x = np.mgrid[0:rows, 0:cols]
        img = 96 + 40 * np.sin(x / 7.0) * np.cos(y / 5.0) + (rng.random((rows, cols)) < 0.02) * 110 + rng.integers(0, 12, (rows, cols))
        for _ in range(max(rows * cols // 300, 4)):
            cy, cx, s = rng.integers(0, rows), rng.integers(0, cols), rng.integers(2, 6)
            img[max(cy - s, 0):cy + s, max(cx - s, 0):cx + s] += rng.integers(-90, 90)
    return np.clip(img, 0, 255).astype(np.uint8)


# name -> (seed, rows, cols, kind, inv_scale, border)
_CASES = {
    "chain_37x53": (1, 37, 53, "noise", CHAIN, 19),
    "halving_40x64": (2, 40, 64, "noise", (F(1), F(.5), F(.25)), 19),
    "halving_cols_only_41x64": (3, 41, 64, "noise", (F(1), F(.5)), 19),      # 64 -> 32, rows 41 -> 20
    "halving_cols_only_43x64": (4, 43, 64, "noise", (F(1), F(.5)), 19),      # 64 -> 32, rows 43 -> 22
    "tile_16x64": (5, 16, 64, "noise", (F(1), Q), 19),
    "tile_17x65": (6, 17, 65, "noise", (F(1), Q), 19),
    "tile_15x63": (7, 15, 63, "noise", (F(1), Q), 19),
    "cols_30x40": (8, 30, 40, "noise", (F(1), Q), 19),
    "cols_30x41": (9, 30, 41, "noise", (F(1), Q), 19),
    "cols_30x42": (10, 30, 42, "noise", (F(1), Q), 19),
    "cols_30x43": (11, 30, 43, "noise", (F(1), Q), 19),
    "clamps_12x20": (12, 12, 20, "noise", (F(1), F(1), F(1.5), F(.75)), 19),
    "one_row_1x50": (13, 1, 50, "noise", (F(1), F(.75)), 19),
    "one_col_50x1": (14, 50, 1, "noise", (F(1), F(.75)), 19),
    "to_one_row_2x50": (15, 2, 50, "noise", (F(1), F(.5)), 19),
    "to_one_col_50x2": (16, 50, 2, "noise", (F(1), F(.5)), 19),
    "tiny_3x3": (17, 3, 3, "noise", (F(1), F(1) / F(3)), 19),
    "border0_9x70": (18, 9, 70, "noise", (F(1),), 0),
    "border3_9x70": (18, 9, 70, "noise", (F(1),), 3),
    "border19_9x70": (18, 9, 70, "noise", (F(1),), 19),
    "zeros_37x53": (0, 37, 53, "zeros", CHAIN, 19),
    "ones_37x53": (0, 37, 53, "ones", CHAIN, 19),
    "ones_clamps_12x20": (0, 12, 20, "ones", (F(1), F(1), F(1.5), F(.75)), 19),
    "checker_37x53": (0, 37, 53, "checker", CHAIN, 19),
    "checker_halving_40x64": (0, 40, 64, "checker", (F(1), F(.5), F(.25)), 19),
}
CASE_NAMES = tuple(_CASES)
VGA = (F(1),) + tuple(F(1) / F(np.float32(1.2) ** l) for l in range(1, 8))


def standin_inv_scale(nlevels: int, scale_factor: float = 1.2):
    """mvInvScaleFactor as the ORBextractor constructor fills it (src/ORBextractor.cc:416-429): float32 products and quotients."""
    sf = [F(1)]
    for _ in range(1, nlevels):
        sf.append(F(sf[-1] * F(scale_factor)))
    return tuple(F(1) / s for s in sf)


def item(name: str) -> dict:
    if name == "vga_752x480_L8":
        return dict(image=image(31, 480, 752, "smooth"), inv_scale=np.asarray(standin_inv_scale(8), F), border=19)
    seed, rows, cols, kind, inv, border = _CASES[name]
    return dict(image=image(seed, rows, cols, kind), inv_scale=np.asarray(inv, F), border=border)


@functools.lru_cache(maxsize=None)
def _expected(name: str):
    it = item(name)
    return build(it["image"], it["inv_scale"], it["border"])


def case(name: str):
    """(item, expected): the item for pyramid_build / pyramid_cpu and dict(levels, bordered) of the restatement."""
    levels, whole = _expected(name)
    return item(name), dict(levels=levels, bordered=whole)


def assert_same(got: dict, exp: dict, what: str, download: bool = True):
    assert got["shapes"] == [lv.shape for lv in exp["levels"]], (what, got["shapes"])
    if not download:
        return
    for l, (g, e) in enumerate(zip(got["bordered"], exp["bordered"])):
        assert g.shape == e.shape, (what, l, g.shape, e.shape)
        bad = np.argwhere(g != e)
        assert bad.size == 0, f"{what}: level {l}: {len(bad)} pixels differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {e[tuple(bad[0])]}"
