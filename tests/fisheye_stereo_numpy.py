"""numpy restatement of Frame::ComputeStereoFishEyeMatches (reference src/Frame.cc:1131-1171) and
KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:306-375 with unproject :116-143, project :67-84 and
Triangulate :394-406) on a synth_fisheye.FisheyeFrame.

One ``np.float32`` operation per float operation of the reference, in its order; Eigen's three-term reductions (dot, norm,
matrix * vector) as a0 + (a1 + a2); sqrtf, tan, atan2f, cos, sin as the float64 function rounded once.  The one deviation, shared
with the device code: the right singular vector of the 4x4 matrix A comes from a float64 decomposition of A's float32 entries
(``numpy.linalg.svd``; ``route="eigh"`` takes it from ``eigh`` of A^T A instead) and x3D = head(3) / w is rounded to float32 once.

A ratio-accepted match is **borderline** when a compared quantity lies within a relative 1e-3 of its threshold: cosParallaxRays
against 0.9998, a squared re-projection error against 5.991 * sigma, z1 against 0.0001, or |z1| or |z2| below 1e-3 * |x3D|.  The
margin is derived: one ulp of x3D (6e-8 relative) moves a projection by about 1e-4 px at these focal lengths, a relative 1e-4 of a
squared error near its threshold of about 6 px^2; 1e-3 is ten times that.
"""
import math

import numpy as np

from orb_slam3_study_kr_amd import capi

F = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)
MARGIN = 1e-3

# name -> synth_fisheye.make_fisheye_frame arguments.  tz > 0 rigs reach OSH_FSTEREO_BEHIND_2, tz < 0 rigs OSH_FSTEREO_DEPTH.
CASES = [
    ("ahead", dict(seed=1, n_left=900, n_right=880, tz=0.04)),
    ("behind", dict(seed=2, n_left=900, n_right=940, tz=-0.03)),
    ("shared", dict(seed=3, n_left=700, n_right=600, tz=0.04, shared=0.25, mono_left=0, mono_right=5)),
    ("mono", dict(seed=4, n_left=800, n_right=800, tz=-0.03, mono_left=300, mono_right=350, wrong=0.15)),
    ("no_pair", dict(seed=5, n_left=70, n_right=40, tz=0.04, mono_left=8, mono_right=39)),
]

# A rig with a pure x-baseline and no distortion (theta_d = theta: a pixel f * angle off the centre looks `angle` off the axis) and
# hand-made pairs on it: name -> (left pixel, right pixel, expected return value (None: a depth), expected point)
FOCAL, CENTRE, BASE, ANGLE = 200.0, 256.0, 0.1, 0.1
PLAIN = np.array([FOCAL, FOCAL, CENTRE, CENTRE, 0, 0, 0, 0], F)
PLAIN_RIG = (PLAIN, PLAIN, 1e-6, 1e-6, np.eye(3, dtype=F), np.array([BASE, 0, 0], F))
KNOWN_PAIRS = {
    "on_axis": ((CENTRE, CENTRE), (CENTRE - FOCAL * ANGLE, CENTRE), None, (0.0, 0.0, BASE / math.tan(ANGLE))),
    "identical_rays": ((300.0, 200.0), (300.0, 200.0), -1.0, None),
    "crossed": ((CENTRE - FOCAL * ANGLE, CENTRE), (CENTRE + FOCAL * ANGLE, CENTRE), -2.0, None),
}


def sum3(a0, a1, a2):
    return F(a0 + F(a1 + a2))


def sqrt_rn(x):
    return F(math.sqrt(float(x)))


def unproject(cam, precision, x, y):
    """:116-143 -> (rx, ry, 1)"""
    cam = np.asarray(cam, F)
    pwx, pwy = F(F(x - cam[2]) / cam[0]), F(F(y - cam[3]) / cam[1])
    scale = F(1)
    theta_d = sqrt_rn(F(F(pwx * pwx) + F(pwy * pwy)))
    half_pi = F(math.pi / 2.0)
    theta_d = min(max(-half_pi, theta_d), half_pi)
    if float(theta_d) > 1e-8:
        theta = theta_d
        for _ in range(10):
            t2 = F(theta * theta); t4 = F(t2 * t2); t6 = F(t4 * t2); t8 = F(t4 * t4)
            k0, k1, k2, k3 = F(cam[4] * t2), F(cam[5] * t4), F(cam[6] * t6), F(cam[7] * t8)
            num = F(F(theta * F(F(F(F(F(1) + k0) + k1) + k2) + k3)) - theta_d)
            den = F(F(F(F(F(1) + F(F(3) * k0)) + F(F(5) * k1)) + F(F(7) * k2)) + F(F(9) * k3))
            fix = F(num / den)
            theta = F(theta - fix)
            if abs(fix) < F(precision):
                break
        scale = F(F(math.tan(float(theta))) / theta_d)
    return F(pwx * scale), F(pwy * scale), F(1)


def project(cam, v):
    """:67-84"""
    cam = np.asarray(cam, F)
    x2y2 = F(F(v[0] * v[0]) + F(v[1] * v[1]))
    theta = F(math.atan2(float(sqrt_rn(x2y2)), float(v[2])))
    psi = F(math.atan2(float(v[1]), float(v[0])))
    t2 = F(theta * theta); t3 = F(theta * t2); t5 = F(t3 * t2); t7 = F(t5 * t2); t9 = F(t7 * t2)
    r = F(F(F(F(theta + F(cam[4] * t3)) + F(cam[5] * t5)) + F(cam[6] * t7)) + F(cam[7] * t9))
    u = F(F(F(cam[0] * r) * F(math.cos(float(psi)))) + cam[2])
    w = F(F(F(cam[1] * r) * F(math.sin(float(psi)))) + cam[3])
    return u, w


def null_vector(A, route="svd"):
    """x3D = head(3) / w of the right singular vector of A's smallest singular value, float64 inside, rounded to float32 once."""
    A64 = np.asarray(A, np.float64)
    if route == "svd":
        h = np.linalg.svd(A64)[2][3]
    else:
        h = np.linalg.eigh(A64.T @ A64)[1][:, 0]
    with np.errstate(all="ignore"):
        return (h[:3] / h[3]).astype(F)


def _near(value, threshold):
    return abs(float(value) - threshold) <= MARGIN * abs(threshold)


def triangulate(rig, p1, p2, sigma1, sigma2, route="svd"):
    """TriangulateMatches -> (return value, x3D, cosParallaxRays, borderline)."""
    cam1, cam2, prec1, prec2, R12, t12 = rig
    R12, t12 = np.asarray(R12, F).reshape(3, 3), np.asarray(t12, F)
    x1, y1, x2, y2 = F(p1[0]), F(p1[1]), F(p2[0]), F(p2[1])
    zero = np.zeros(3, F)
    with np.errstate(all="ignore"):
        r1 = unproject(cam1, prec1, x1, y1)
        r2 = unproject(cam2, prec2, x2, y2)
        r21 = [sum3(F(R12[i, 0] * r2[0]), F(R12[i, 1] * r2[1]), F(R12[i, 2] * r2[2])) for i in range(3)]
        dot = sum3(F(r1[0] * r21[0]), F(r1[1] * r21[1]), F(r1[2] * r21[2]))
        n1 = sqrt_rn(sum3(F(r1[0] * r1[0]), F(r1[1] * r1[1]), F(r1[2] * r1[2])))
        n21 = sqrt_rn(sum3(F(r21[0] * r21[0]), F(r21[1] * r21[1]), F(r21[2] * r21[2])))
        cosp = F(dot / F(n1 * n21))
        border = _near(cosp, 0.9998)
        if float(cosp) > 0.9998:
            return F(-1), zero, cosp, border
        T2 = np.zeros((3, 4), F)
        for i in range(3):
            for j in range(3):
                T2[i, j] = R12[j, i]
            T2[i, 3] = -sum3(F(T2[i, 0] * t12[0]), F(T2[i, 1] * t12[1]), F(T2[i, 2] * t12[2]))
        A = np.zeros((4, 4), F)
        A[0] = [-1, 0, r1[0], 0]
        A[1] = [0, -1, r1[1], 0]
        for j in range(4):
            A[2, j] = F(F(r2[0] * T2[2, j]) - T2[0, j])
            A[3, j] = F(F(r2[1] * T2[2, j]) - T2[1, j])
        x3D = null_vector(A, route)
        z1 = x3D[2]
        z2 = F(sum3(F(T2[2, 0] * x3D[0]), F(T2[2, 1] * x3D[1]), F(T2[2, 2] * x3D[2])) + T2[2, 3])
        norm = float(np.linalg.norm(x3D.astype(np.float64)))
        border = border or abs(float(z1)) < MARGIN * norm or abs(float(z2)) < MARGIN * norm
        if z1 <= 0:
            return F(-2), zero, cosp, border
        if z2 <= 0:
            return F(-3), zero, cosp, border
        u1, v1 = project(cam1, x3D)
        ex, ey = F(u1 - x1), F(v1 - y1)
        e1 = F(F(ex * ex) + F(ey * ey))
        border = border or _near(e1, 5.991 * float(F(sigma1)))
        if float(e1) > 5.991 * float(F(sigma1)):
            return F(-4), zero, cosp, border
        x3D2 = [F(sum3(F(T2[i, 0] * x3D[0]), F(T2[i, 1] * x3D[1]), F(T2[i, 2] * x3D[2])) + T2[i, 3]) for i in range(3)]
        u2, v2 = project(cam2, x3D2)
        ex, ey = F(u2 - x2), F(v2 - y2)
        e2 = F(F(ex * ex) + F(ey * ey))
        border = border or _near(e2, 5.991 * float(F(sigma2)))
        if float(e2) > 5.991 * float(F(sigma2)):
            return F(-5), zero, cosp, border
        border = border or _near(z1, float(F(0.0001)))
        return z1, x3D, cosp, border


def rig_of(fr):
    return fr.cam1, fr.cam2, fr.precision1, fr.precision2, fr.Rlr, fr.tlr


def knn2(fr):
    """The two smallest Hamming distances of every left keypoint >= mono_left among the right ones >= mono_right and the index of the
    smallest (the lowest index among equal distances); -1 everywhere for keypoints that are no query or have no pair."""
    n = fr.left_xy.shape[0]
    best = np.full(n, -1, np.int32); d0 = np.full(n, -1, np.int32); d1 = np.full(n, -1, np.int32)
    train = fr.right_desc[fr.mono_right:]
    if train.shape[0] < 2:
        return best, d0, d1
    for a in range(fr.mono_left, n, 256):
        q = fr.left_desc[a:a + 256]
        dist = _POP[q[:, None, :] ^ train[None, :, :]].sum(axis=2)
        i0 = dist.argmin(axis=1)
        rows = np.arange(q.shape[0])
        d0[a:a + 256] = dist[rows, i0]
        dist[rows, i0] = 1 << 20
        d1[a:a + 256] = dist.min(axis=1)
        best[a:a + 256] = i0 + fr.mono_right
    return best, d0, d1


_RET_STAGE = {-1: capi.OSH_FSTEREO_PARALLAX, -2: capi.OSH_FSTEREO_BEHIND_1, -3: capi.OSH_FSTEREO_BEHIND_2,
              -4: capi.OSH_FSTEREO_REPROJ_1, -5: capi.OSH_FSTEREO_REPROJ_2}


def compute(fr, route="svd") -> dict:
    """The outputs of osh_fisheye_stereo_result plus `borderline` [n_left] and `ratio_ok` [n_left]."""
    n, nr = fr.left_xy.shape[0], fr.right_xy.shape[0]
    best, d0, d1 = knn2(fr)
    out = dict(left_to_right=np.full(n, -1, np.int32), right_to_left=np.full(nr, -1, np.int32), depth=np.full(n, -1, F),
               p3d=np.zeros((n, 3), F), best_right=best, best_dist=d0, second_dist=d1,
               cos_parallax=np.full(n, capi.OSH_FSTEREO_NO_COS, F), stage=np.zeros(n, np.uint8), borderline=np.zeros(n, bool),
               ratio_ok=np.zeros(n, bool))
    rig = rig_of(fr)
    sig = np.asarray(fr.level_sigma2, F)
    for l in range(n):
        if l < fr.mono_left:
            out["stage"][l] = capi.OSH_FSTEREO_OUTSIDE
        elif nr - fr.mono_right < 2:
            out["stage"][l] = capi.OSH_FSTEREO_NO_PAIR
        elif not float(F(d0[l])) < float(F(d1[l])) * 0.7:
            out["stage"][l] = capi.OSH_FSTEREO_RATIO
        else:
            r = int(best[l])
            out["ratio_ok"][l] = True
            ret, x3D, cosp, border = triangulate(rig, fr.left_xy[l], fr.right_xy[r], sig[fr.left_octave[l]], sig[fr.right_octave[r]], route)
            out["cos_parallax"][l] = cosp
            out["borderline"][l] = border
            if float(ret) in _RET_STAGE:
                out["stage"][l] = _RET_STAGE[float(ret)]
            elif not ret > F(0.0001):
                out["stage"][l] = capi.OSH_FSTEREO_DEPTH
            else:
                out["stage"][l] = capi.OSH_FSTEREO_ACCEPTED
                out["left_to_right"][l] = r
                out["right_to_left"][r] = l          # ascending l: the last writer stays
                out["depth"][l] = ret
                out["p3d"][l] = x3D
    return out


def ulp_distance(a, b) -> np.ndarray:
    """Number of float32 values between a and b (0: equal bits up to the sign of zero)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def right_to_left_of(left_to_right, n_right) -> np.ndarray:
    """mvRightToLeftMatch of a set of accepted matches: the largest l that names r."""
    out = np.full(n_right, -1, np.int32)
    for l, r in enumerate(left_to_right):
        if r >= 0:
            out[r] = l
    return out


def assert_matches(got: dict, exp: dict, what: str = ""):
    """The comparison of the GPU tests: bit for bit up to A, depth / p3d within one float32 step where both accept, stage and the
    match arrays equal wherever the restatement is not borderline (a borderline match may take one test the other way)."""
    for k in ("best_right", "best_dist", "second_dist"):
        assert np.array_equal(got[k], exp[k]), f"{what}: {k} differs at {np.nonzero(got[k] != exp[k])[0][:8]}"
    ratio_got = got["stage"] >= capi.OSH_FSTEREO_PARALLAX
    assert np.array_equal(ratio_got, exp["ratio_ok"]), f"{what}: ratio decision differs"
    cg, ce = np.ascontiguousarray(got["cos_parallax"], F).view(np.uint32), np.ascontiguousarray(exp["cos_parallax"], F).view(np.uint32)
    assert np.array_equal(cg, ce), f"{what}: cos_parallax bits differ at {np.nonzero(cg != ce)[0][:8]}"
    firm = ~exp["borderline"]
    bad = np.nonzero((got["stage"] != exp["stage"]) & firm)[0]
    assert bad.size == 0, f"{what}: stage differs at {bad[:8]}: {got['stage'][bad[:8]]} vs {exp['stage'][bad[:8]]}"
    soft = np.nonzero((got["stage"] != exp["stage"]) & ~firm)[0]   # one test decided the other way; what follows it is free
    assert np.array_equal(got["left_to_right"][firm], exp["left_to_right"][firm]), f"{what}: left_to_right"
    both = (got["stage"] == capi.OSH_FSTEREO_ACCEPTED) & (exp["stage"] == capi.OSH_FSTEREO_ACCEPTED)
    du = ulp_distance(got["depth"][both], exp["depth"][both])
    pu = ulp_distance(np.asarray(got["p3d"], F).reshape(-1, 3)[both], exp["p3d"][both])
    assert du.size == 0 or (du.max() <= 1 and pu.max() <= 1), f"{what}: depth {du.max()} ulp, p3d {pu.max()} ulp"
    acc = got["stage"] == capi.OSH_FSTEREO_ACCEPTED
    assert np.array_equal(got["left_to_right"] >= 0, acc) and np.array_equal(got["depth"] > 0, acc), f"{what}: accepted set"
    # right keypoints that no borderline left keypoint names are settled by firm matches alone
    settled = np.ones(exp["right_to_left"].shape[0], bool)
    named = exp["best_right"][exp["borderline"]]
    settled[named[named >= 0]] = False
    assert np.array_equal(got["right_to_left"][settled], exp["right_to_left"][settled]), f"{what}: right_to_left"
    assert np.array_equal(got["right_to_left"], right_to_left_of(got["left_to_right"], got["right_to_left"].shape[0])), \
        f"{what}: right_to_left is not the largest accepted l"


def assert_same(a: dict, b: dict, what: str = ""):
    """Two device results, bit for bit."""
    for k in ("left_to_right", "right_to_left", "best_right", "best_dist", "second_dist", "stage"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"
    for k in ("depth", "p3d", "cos_parallax"):
        assert np.array_equal(np.ascontiguousarray(a[k], F).view(np.uint32), np.ascontiguousarray(b[k], F).view(np.uint32)), f"{what}: {k}"
