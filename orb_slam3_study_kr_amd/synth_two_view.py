"""Deterministic two-view scenes for TwoViewReconstruction (the monocular initialisation): float32 pixels of two frames with noise
and an outlier share, more keypoints than matches (Normalize runs over all keypoints of a frame), and matches whose idx2 is a
permutation (the scatter into vKeys1 order is exercised).  A Scene is what TwoViewReconstruction::Reconstruct takes; problem() turns
it into what osh_orb_two_view_reconstruct takes: the matches in mvMatches12 order (ascending idx1), the two Normalize results and the
minimal sets.

Named cases (CASES): general (depth spread: F wins and is accepted), planar (a tilted plane: H wins and is accepted), rotation
(near-zero baseline: rejected for parallax), ambiguous (a far scene with a short baseline: several motion hypotheses count most
points, no clear winner), sparse (too few inliers), coincident (four correspondences repeated: every minimal set is degenerate), coincident_accepted (the same kind with 120
matches, the four points on the planar case's plane and a sideways baseline of 2: the homography is the plane's, four
correspondences pin no fundamental matrix, so H wins, and Faugeras' second solution keeps only half of the points in front of both
cameras, so ReconstructH accepts the true motion).
"""
import dataclasses

import numpy as np

F = np.float32
WIDTH, HEIGHT = 640.0, 480.0


@dataclasses.dataclass
class Scene:
    name: str
    K: np.ndarray            # [3, 3] float32
    sigma: float
    keys1: np.ndarray        # [n1, 2] float32
    keys2: np.ndarray        # [n2, 2] float32
    matches12: np.ndarray    # [n1] int32, -1: unmatched
    R: np.ndarray            # [3, 3] float64: x2 = R x1 + t
    t: np.ndarray            # [3] float64
    kb8: np.ndarray = None   # [8] float32 fx fy cx cy k1..k4 when the pixels are fisheye pixels


@dataclasses.dataclass
class Problem:
    name: str
    K: np.ndarray
    sigma: float
    n_keys1: int
    n_keys2: int
    idx1: np.ndarray         # [n] int32
    idx2: np.ndarray
    pt1: np.ndarray          # [n, 2] float32
    pt2: np.ndarray
    T1: np.ndarray           # [3, 3] float32
    T2: np.ndarray
    pn1: np.ndarray          # [n, 2] float32
    pn2: np.ndarray
    sets: np.ndarray         # [n_iterations, 8] int32

    @property
    def n(self):
        return int(self.idx1.shape[0])

    @property
    def n_iterations(self):
        return int(self.sets.shape[0])


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def normalize(xy):
    """Normalize (src/TwoViewReconstruction.cc:737-784) over all keypoints xy [n, 2]: (pn [n, 2], T [3, 3]), float32.  The sums are
    sequential float32 chains in index order (numpy's accumulate adds one element after another)."""
    xy = np.ascontiguousarray(xy, F)
    n = xy.shape[0]
    chain = lambda a: np.add.accumulate(a, dtype=F)[-1] if a.shape[0] else F(0)
    mean = np.array([F(chain(xy[:, 0]) / F(n)), F(chain(xy[:, 1]) / F(n))], F)
    pn = (xy - mean).astype(F)
    dev = np.array([F(chain(np.abs(pn[:, 0])) / F(n)), F(chain(np.abs(pn[:, 1])) / F(n))], F)
    s = np.array([F(1.0 / float(dev[0])), F(1.0 / float(dev[1]))], F)
    pn = (pn * s).astype(F)
    T = np.zeros((3, 3), F)
    T[0, 0], T[1, 1], T[2, 2] = s[0], s[1], F(1)
    T[0, 2], T[1, 2] = F(-mean[0]) * s[0], F(-mean[1]) * s[1]
    return pn, T


def draw_sets(rng, n, n_iterations):
    """n_iterations minimal sets of 8 distinct match indices [n_iterations, 8]; with n == 8 every set is a permutation of all."""
    return np.array([rng.permutation(n)[:8] for _ in range(n_iterations)], np.int32).reshape(n_iterations, 8)


def problem(scene: Scene, n_iterations: int = 200, seed: int = 0, head: int = None, sets=None) -> Problem:
    """The C-ABI view of a scene.  head: keep only the first `head` matches (the keypoints of both frames stay, so the Normalize
    results do not change)."""
    idx1 = np.nonzero(scene.matches12 >= 0)[0].astype(np.int32)
    if head is not None:
        idx1 = idx1[:head]
    idx2 = scene.matches12[idx1].astype(np.int32)
    pn1, T1 = normalize(scene.keys1)
    pn2, T2 = normalize(scene.keys2)
    if sets is None:
        sets = draw_sets(np.random.default_rng([seed, idx1.shape[0], n_iterations]), idx1.shape[0], n_iterations) if n_iterations else np.zeros((0, 8), np.int32)
    return Problem(scene.name, scene.K.astype(F), float(scene.sigma), scene.keys1.shape[0], scene.keys2.shape[0], idx1, idx2,
                   np.ascontiguousarray(scene.keys1[idx1], F), np.ascontiguousarray(scene.keys2[idx2], F), T1, T2,
                   np.ascontiguousarray(pn1[idx1], F), np.ascontiguousarray(pn2[idx2], F), np.ascontiguousarray(sets, np.int32))


def kb8_project(cam, X):
    """KannalaBrandt8::project (src/CameraModels/KannalaBrandt8.cpp:45-63) in float64 for points X [n, 3]."""
    theta = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2])
    psi = np.arctan2(X[:, 1], X[:, 0])
    r = theta + cam[4] * theta ** 3 + cam[5] * theta ** 5 + cam[6] * theta ** 7 + cam[7] * theta ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], 1)


def make_scene(kind: str, seed: int = 0, n: int = 300, extra: int = 40, noise: float = 0.25, outliers: float = 0.1, fisheye: bool = False,
               outlier_spread: float = None, on_plane: bool = False, plane=(0.35, -0.2), t_override=None) -> Scene:
    """kind: see the module text.  outlier_spread: None puts a wrong match anywhere in the image, a number that many pixels (sigma)
    from the right place.  on_plane: take the points from the plane z = 5 + plane[0] x + plane[1] y (the planar kind always does).
    t_override: a baseline in place of the kind's."""
    rng = np.random.default_rng([seed, n, sum(map(ord, kind))])
    K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], np.float64)
    R, t = rotation(0.02, 0.08, -0.03), np.array([0.6, 0.05, 0.1])
    distinct = n
    if kind == "planar":
        R, t = rotation(0.03, -0.1, 0.02), np.array([0.5, -0.1, 0.15])
    elif kind == "rotation":
        t = np.array([0.05, 0.008, 0.0])
    elif kind == "ambiguous":
        t = np.array([0.02, 0.0, 0.0])
    elif kind == "sparse":
        outliers = 0.85
    elif kind == "coincident":
        distinct, noise, outliers = 4, 0.0, 0.0
    elif kind != "general":
        raise ValueError(kind)
    if t_override is not None:
        t = np.asarray(t_override, np.float64)
    # points in front of both cameras whose pixels fall inside both images
    X = np.zeros((0, 3))
    while X.shape[0] < distinct:
        c = np.stack([rng.uniform(-3, 3, 4 * n), rng.uniform(-2.2, 2.2, 4 * n), rng.uniform(2.5, 9.0, 4 * n)], 1)
        if kind == "rotation":      # parallax between 0.57 and 1.15 degrees: above the 0.99998 cosine, fewer than 50 points above 1 degree
            c[:, 2] = rng.uniform(2.5, 5.0, 4 * n)
        if kind == "planar" or on_plane:
            c[:, 2] = 5.0 + plane[0] * c[:, 0] + plane[1] * c[:, 1]
        elif kind == "ambiguous":
            c[:, 2] = rng.uniform(40.0, 60.0, 4 * n)
            c[:, :2] *= c[:, 2:3] / 6.0
        c2 = c @ R.T + t
        ok = (c[:, 2] > 0.5) & (c2[:, 2] > 0.5)
        for pts in (c, c2):
            uv = pts[:, :2] / pts[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
            ok &= (uv[:, 0] > 8) & (uv[:, 0] < WIDTH - 8) & (uv[:, 1] > 8) & (uv[:, 1] < HEIGHT - 8)
        X = np.concatenate([X, c[ok]])[:distinct]
    X = X[np.arange(n) % distinct]
    X2 = X @ R.T + t
    cam = np.array([500, 500, 320, 240, -0.02, 0.004, -0.001, 0.0002])
    if fisheye:
        p1, p2 = kb8_project(cam, X), kb8_project(cam, X2)
    else:
        p1 = X[:, :2] / X[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
        p2 = X2[:, :2] / X2[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    p1 = p1 + rng.normal(0, noise, p1.shape)
    p2 = p2 + rng.normal(0, noise, p2.shape)
    bad = rng.random(n) < outliers
    if outlier_spread is None:   # a wrong match anywhere in the image
        p2[bad] = np.stack([rng.uniform(8, WIDTH - 8, bad.sum()), rng.uniform(8, HEIGHT - 8, bad.sum())], 1)
    else:                        # a wrong match to a neighbouring feature
        p2[bad] += rng.normal(0, outlier_spread, (int(bad.sum()), 2))
    n1, n2 = n + extra, n + extra + 7
    pos1 = np.sort(rng.permutation(n1)[:n])
    pos2 = rng.permutation(n2)[:n]
    keys1 = np.stack([rng.uniform(8, WIDTH - 8, n1), rng.uniform(8, HEIGHT - 8, n1)], 1)
    keys2 = np.stack([rng.uniform(8, WIDTH - 8, n2), rng.uniform(8, HEIGHT - 8, n2)], 1)
    keys1[pos1], keys2[pos2] = p1, p2
    matches12 = np.full(n1, -1, np.int32)
    matches12[pos1] = pos2
    return Scene(kind, K.astype(F), 1.0, keys1.astype(F), keys2.astype(F), matches12, R, t, cam.astype(F) if fisheye else None)


# name -> make_scene arguments
CASES = {
    "general": dict(kind="general", seed=1),
    "planar": dict(kind="planar", seed=2),
    "rotation": dict(kind="rotation", seed=3),
    "ambiguous": dict(kind="ambiguous", seed=4),
    "sparse": dict(kind="sparse", seed=5, n=120),
    "coincident": dict(kind="coincident", seed=6, n=40),
    "coincident_accepted": dict(kind="coincident", seed=1, n=120, on_plane=True, t_override=(2.0, 0.0, 0.0)),
}
