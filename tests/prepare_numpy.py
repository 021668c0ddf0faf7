"""The image front end as include/orbslam3_hip.h defines it (remap or resize on every channel, then grey), restated in numpy: integer
arithmetic in int64, float32 only for mx * 32 with np.rint.  The resize is pyramid_numpy's.  It shares no code with
csrc/orb_prepare.h.  case(name) yields the committed cases: an item (image, order, maps, sizes) and the expected grey image.

rectify_maps is a pinhole-plus-radial camera model evaluated in float64 and cast to float32, the kind of map
initUndistortRectifyMap produces: written from the textbook model (normalise by the new camera, rotate back, distort with two
radial and two tangential coefficients, project with the old camera)."""
import functools

import numpy as np

import pyramid_numpy as pn

F = np.float32
I = np.int64


def rectify_maps(rows, cols, src_shape, f=0.9, k1=-0.28, k2=0.07, p1=3e-4, p2=-2e-4, tilt=0.01, shift=(0.0, 0.0), zoom=0.8):
    """map_x, map_y (float32 [rows, cols]): where destination pixel (y, x) of a rows x cols rectified image lies in a source image
    of src_shape.  f: focal length over the source width; tilt: a rotation about x and y in radians; shift: the principal point's
    offset from the source centre in pixels; zoom: the new focal length over the old one, per output width (below 1 the corners of
    the output look past the source)."""
    sr, sc = src_shape
    fx = fy = np.float64(f) * sc
    cx, cy = (sc - 1) / 2.0 + shift[0], (sr - 1) / 2.0 + shift[1]
    nfx = nfy = np.float64(f) * cols * zoom
    ncx, ncy = (cols - 1) / 2.0, (rows - 1) / 2.0
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ray = np.stack([(u - ncx) / nfx, (v - ncy) / nfy, np.ones_like(u)], -1)
    ca, sa, cb, sb = np.cos(tilt), np.sin(tilt), np.cos(-tilt / 2), np.sin(-tilt / 2)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    ray = ray @ (Ry @ Rx)          # the inverse rotation applied to row vectors
    x, y = ray[..., 0] / ray[..., 2], ray[..., 1] / ray[..., 2]
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return (fx * xd + cx).astype(F), (fy * yd + cy).astype(F)


def remap(src: np.ndarray, map_x: np.ndarray, map_y: np.ndarray) -> np.ndarray:
    """src [rows, cols, channels] -> [map rows, map cols, channels], int64."""
    S = src.astype(I)
    rows, cols = S.shape[:2]
    mx, my = map_x.astype(F), map_y.astype(F)
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(mx) & np.isfinite(my) & (np.abs(mx) <= F(32768)) & (np.abs(my) <= F(32768))
    sx = np.rint(np.where(usable, mx, F(0)) * F(32)).astype(I)
    sy = np.rint(np.where(usable, my, F(0)) * F(32)).astype(I)
    ix, fx, iy, fy = sx >> 5, (sx & 31)[..., None], sy >> 5, (sy & 31)[..., None]

    def p(r, c):
        inside = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
        return np.where(inside[..., None], S[np.clip(r, 0, rows - 1), np.clip(c, 0, cols - 1)], 0)

    top = (32 - fx) * p(iy, ix) + fx * p(iy, ix + 1)
    bottom = (32 - fx) * p(iy + 1, ix) + fx * p(iy + 1, ix + 1)
    out = ((32 - fy) * top + fy * bottom + 512) >> 10
    return np.where(usable[..., None], out, 0)


def resize(src: np.ndarray, rows: int, cols: int) -> np.ndarray:
    return np.stack([pn.resample(src[..., ch].astype(np.uint8), rows, cols) for ch in range(src.shape[2])], -1).astype(I)


def gray(v: np.ndarray, order: str) -> np.ndarray:
    """v [rows, cols, channels] int64 -> uint8 [rows, cols]."""
    if v.shape[2] == 1:
        return v[..., 0].astype(np.uint8)
    r, b = (v[..., 0], v[..., 2]) if order == "rgb" else (v[..., 2], v[..., 0])
    return ((r * 4899 + v[..., 1] * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def prepare(it: dict) -> np.ndarray:
    """The grey image of an item: geometry on every channel, then grey."""
    img = it["image"]
    src = (img[..., None] if img.ndim == 2 else img).astype(I)
    if it.get("map_x") is not None:
        v = remap(src, it["map_x"], it["map_y"])
    elif it.get("out_shape") is not None and tuple(it["out_shape"]) != img.shape[:2]:
        v = resize(src, *it["out_shape"])
    else:
        v = src
    return gray(v, it.get("order", "rgb"))


def noise(seed, rows, cols, channels=1):
    a = np.random.default_rng(seed).integers(0, 256, (rows, cols, channels)).astype(np.uint8)
    return a[..., 0] if channels == 1 else a


def identity_maps(rows, cols, dx=0.0, dy=0.0):
    y, x = np.mgrid[0:rows, 0:cols]
    return (x + dx).astype(F), (y + dy).astype(F)


def edge_maps():
    """12 x 20 maps onto a 12 x 20 source: a smooth base, and single pixels set by hand to the edges of the definition."""
    mx, my = rectify_maps(12, 20, (12, 20))
    put = [  # (y, x, mx, my)
        (0, 0, -1 / 32, 3.0),            # sx = -1: ix = -1, fx = 31
        (0, 1, 19.25, 2.0),              # ix = cols - 1: the second tap is outside
        (0, 2, 4.0, -1.5),               # iy = -2: both rows outside
        (0, 3, 100.0, 100.0),            # fully outside
        (0, 4, 64.5 / 32, 5.0),          # mx * 32 = 64.5 exactly: to 64
        (0, 5, 65.5 / 32, 5.0),          # mx * 32 = 65.5 exactly: to 66
        (0, 6, np.nan, 5.0), (0, 7, np.inf, 5.0), (0, 8, 40000.0, 5.0), (0, 9, 5.0, np.nan), (0, 10, -40000.0, 5.0),
        (0, 11, 32768.0, 5.0),           # usable, and outside
        (0, 12, 5.0, -np.inf), (0, 13, -32768.0, -32768.0),
        (1, 0, 7.0, 11.5),               # iy = rows - 1: the second row is outside
        (1, 1, -16.5 / 32, 4.0),         # mx * 32 = -16.5 exactly: to -16, ix = -1, fx = 16
        (1, 2, 19.0, 11.0),              # the last pixel, no fraction
        (1, 3, -1.0, -1.0),              # ix = iy = -1, no fraction: every tap outside or weightless
        (11, 19, 19.96875, 11.96875),    # fx = fy = 31 on the last pixel
        (11, 18, 5.0, 32769.0),          # just beyond usable
    ]
    for y, x, a, b in put:
        mx[y, x], my[y, x] = F(a), F(b)
    return mx, my


def _colours(seed, order, channels):
    """5 x 7 random bytes; the first row starts with pure red, green, blue and white in the item's channel order."""
    img = noise(seed, 5, 7, channels)
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8)
    img[0, :4, :3] = rgb if order == "rgb" else rgb[:, ::-1]
    return img


@functools.lru_cache(maxsize=None)
def item(name: str) -> dict:
    """image, order, map_x / map_y or None, out_shape or None.  Arrays are shared: do not write into them."""
    def with_map(img, maps, order="rgb"):
        return dict(image=img, order=order, map_x=maps[0], map_y=maps[1], out_shape=None)

    def plain(img, out_shape=None, order="rgb"):
        return dict(image=img, order=order, map_x=None, map_y=None, out_shape=out_shape)

    if name == "remap_17x65_from_23x70":
        return with_map(noise(1, 23, 70), rectify_maps(17, 65, (23, 70)))
    if name == "remap_edges_12x20":
        return with_map(noise(2, 12, 20), edge_maps())
    if name == "identity_9x70":
        return with_map(noise(3, 9, 70), identity_maps(9, 70))
    if name == "half_pixel_8x8":
        return with_map(noise(4, 8, 8), identity_maps(8, 8, 0.5, 0.5))
    if name in ("gray_rgb_5x7", "gray_bgr_5x7", "gray_rgba_5x7", "gray_bgra_5x7"):
        order = "rgb" if "rgb" in name else "bgr"
        return plain(_colours(5, order, 4 if "a_" in name else 3), order=order)
    if name == "rgb_remap_37x53":
        return with_map(noise(6, 41, 57, 3), rectify_maps(37, 53, (41, 57)))
    if name.startswith("resize_40x64_to_20x32"):
        return plain(noise(7, 40, 64, int(name[-1])), (20, 32), "bgr")
    if name.startswith("resize_37x53_to_30x41"):
        return plain(noise(8, 37, 53, int(name[-1])), (30, 41))
    if name == "passthrough_1x50":
        return plain(noise(9, 1, 50))
    if name == "euroc_752x480":
        return with_map(pn.image(31, 480, 752, "smooth"), rectify_maps(480, 752, (480, 752), f=0.61, shift=(4.3, -2.6)))
    raise KeyError(name)


CASE_NAMES = ("remap_17x65_from_23x70", "remap_edges_12x20", "identity_9x70", "half_pixel_8x8", "gray_rgb_5x7", "gray_bgr_5x7",
              "gray_rgba_5x7", "gray_bgra_5x7", "rgb_remap_37x53", "resize_40x64_to_20x32_c1", "resize_40x64_to_20x32_c3",
              "resize_37x53_to_30x41_c1", "resize_37x53_to_30x41_c3", "passthrough_1x50")
LARGE = "euroc_752x480"


@functools.lru_cache(maxsize=None)
def expected(name: str) -> np.ndarray:
    out = prepare(item(name))
    out.setflags(write=False)
    return out


def case(name: str):
    """(item, expected grey image)."""
    return item(name), expected(name)


def check_known_answers():
    """What the definition fixes about the committed cases, from the restatement alone."""
    it, exp = case("identity_9x70")
    assert (exp == it["image"]).all()
    it, exp = case("half_pixel_8x8")
    s = it["image"].astype(I)
    assert (exp[:-1, :-1] == ((s[:-1, :-1] + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:] + 2) >> 2)).all()
    assert (exp[-1, :-1] == ((s[-1, :-1] + s[-1, 1:] + 2) >> 2)).all()       # the row below is outside: 0
    for name in ("gray_rgb_5x7", "gray_bgr_5x7", "gray_rgba_5x7", "gray_bgra_5x7"):
        assert expected(name)[0, :4].tolist() == [76, 150, 29, 255], name
    assert (expected("gray_rgb_5x7") != expected("gray_bgr_5x7")).any()
    it, exp = case("passthrough_1x50")
    assert (exp == it["image"]).all()
    # geometry first, then grey: the other order gives another image
    it, exp = case("rgb_remap_37x53")
    first = gray(it["image"].astype(I), "rgb")
    swapped = gray(remap(first[..., None], it["map_x"], it["map_y"]), "rgb")
    assert (swapped != exp).any()
    # the hand-set pixels of the edge case
    it, exp = case("remap_edges_12x20")
    s = it["image"].astype(I)
    assert exp[0, 0] == (31 * s[3, 0] * 32 + 512) >> 10          # ix = -1, fx = 31: only the second tap is inside
    assert exp[0, 1] == (24 * s[2, 19] * 32 + 512) >> 10         # fx = 8 on the last column
    assert exp[0, 2] == 0 and exp[0, 3] == 0
    assert exp[0, 4] == s[5, 2] and exp[0, 5] == (30 * s[5, 2] + 2 * s[5, 3] + 16) >> 5
    assert exp[0, 6:14].tolist() == [0] * 8
    assert exp[1, 0] == (16 * s[11, 7] * 32 + 512) >> 10
    assert exp[1, 1] == (16 * s[4, 0] * 32 + 512) >> 10
    assert exp[1, 2] == s[11, 19] and exp[1, 3] == 0
    assert exp[11, 19] == (s[11, 19] + 512) >> 10 and exp[11, 18] == 0
    # the smooth maps leave the source on some side: the border is exercised by generated maps too
    for name in ("remap_17x65_from_23x70", "rgb_remap_37x53", LARGE):
        it = item(name)
        r, c = it["image"].shape[:2]
        assert ((it["map_x"] < 0) | (it["map_x"] > c - 1) | (it["map_y"] < 0) | (it["map_y"] > r - 1)).any(), name


def assert_same(got: np.ndarray, exp: np.ndarray, what: str):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {exp[tuple(bad[0])]}"
