"""numpy restatement of TwoViewReconstruction (reference src/TwoViewReconstruction.cc) stage by stage, on a synth_two_view.Problem:
the systems of ComputeH21 / ComputeF21 (:232-308), the models of a minimal set, CheckHomography / CheckFundamental (:310-473), the
RANSAC choice (:155-178,206-229), the branch (:112-128), CheckRT (:786-901) and the decisions of ReconstructF / ReconstructH
(:505-568,693-733).

One ``np.float32`` operation per float operation of the reference, in its order (the per-match statements as float32 array
operations over the matches, which are the same IEEE operations element by element); Eigen's three-term reductions as a0 + (a1 + a2);
the score as the sequential float32 sum in match order (numpy's accumulate); sqrt and acos as the float64 function rounded once;
comparisons in double where the reference compares with a double literal.  Singular vectors come from ``numpy.linalg.svd`` in float64
on the float32 entries and are rounded to float32 once; .inverse() is the float32 cofactor inverse csrc/two_view.h defines.

Every stage takes its inputs as arguments, so a test can hand it the previous stage's output of the build under test: the scores
from that build's models, CheckRT from that build's (R, t).  A match is **borderline** for a comparison when the quantity lies
within the relative MARGIN of tests/newpoints_numpy.py of what it is compared with (nn._near).
"""
import math

import numpy as np

import newpoints_numpy as nn
from orb_slam3_study_kr_amd import capi

F = np.float32
MARGIN = nn.MARGIN
bits, ulp_distance = nn.bits, nn.ulp_distance


def f32(x):
    return np.asarray(x, F)


def sum3(a0, a1, a2):
    return f32(a0 + f32(a1 + a2))


def mul3(A, B):
    A, B = f32(A), f32(B)
    C = np.zeros((3, 3), F)
    for i in range(3):
        for j in range(3):
            C[i, j] = sum3(F(A[i, 0] * B[0, j]), F(A[i, 1] * B[1, j]), F(A[i, 2] * B[2, j]))
    return C


def inverse3(M):
    m = f32(M).reshape(9)
    c00 = F(F(m[4] * m[8]) - F(m[5] * m[7]))
    c01 = F(F(m[5] * m[6]) - F(m[3] * m[8]))
    c02 = F(F(m[3] * m[7]) - F(m[4] * m[6]))
    det = sum3(F(m[0] * c00), F(m[1] * c01), F(m[2] * c02))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invdet = F(F(1) / det)
        inv = np.zeros(9, F)
        inv[0], inv[3], inv[6] = F(c00 * invdet), F(c01 * invdet), F(c02 * invdet)
        inv[1] = F(F(F(m[2] * m[7]) - F(m[1] * m[8])) * invdet)
        inv[4] = F(F(F(m[0] * m[8]) - F(m[2] * m[6])) * invdet)
        inv[7] = F(F(F(m[1] * m[6]) - F(m[0] * m[7])) * invdet)
        inv[2] = F(F(F(m[1] * m[5]) - F(m[2] * m[4])) * invdet)
        inv[5] = F(F(F(m[2] * m[3]) - F(m[0] * m[5])) * invdet)
        inv[8] = F(F(F(m[0] * m[4]) - F(m[1] * m[3])) * invdet)
    return inv.reshape(3, 3)


# ---------------------------------------------------------------------------------------------------- models of a minimal set
def system(model, p1, p2):
    """A of ComputeH21 (model 0, [16, 9]) or ComputeF21 (model 1, [8, 9]) for the normalised points p1, p2 [8, 2], float32."""
    u1, v1, u2, v2 = f32(p1[:, 0]), f32(p1[:, 1]), f32(p2[:, 0]), f32(p2[:, 1])
    one, zero = np.ones(8, F), np.zeros(8, F)
    if model == 0:
        even = np.stack([zero, zero, zero, -u1, -v1, -one, f32(v2 * u1), f32(v2 * v1), v2], 1)
        odd = np.stack([u1, v1, one, zero, zero, zero, f32(-u2 * u1), f32(-u2 * v1), -u2], 1)
        return np.stack([even, odd], 1).reshape(16, 9).astype(F)
    return np.stack([f32(u2 * u1), f32(u2 * v1), u2, f32(v2 * u1), f32(v2 * v1), v2, u1, v1, one], 1).astype(F)


def singular_gap(A):
    """(sigma8 - sigma9) / sigma1 of the float32 system in float64: below 1e-6 the null vector is not defined at this precision."""
    s = np.linalg.svd(np.asarray(A, np.float64), compute_uv=False)
    s = np.concatenate([s, np.zeros(9 - s.shape[0])])
    return (s[7] - s[8]) / s[0] if s[0] > 0 else 0.0


def null_vector(A):
    """The right singular vector of the smallest singular value (float64 LAPACK), rounded to float32 once; the sign is free."""
    return np.linalg.svd(np.asarray(A, np.float64), full_matrices=True)[2][8].astype(F)


def rank2(Fpre):
    u, w, vt = np.linalg.svd(np.asarray(Fpre, np.float64).reshape(3, 3))
    return ((u[:, :2] * w[:2]) @ vt[:2]).astype(F)


def normalised_model(model, h):
    return f32(h).reshape(3, 3) if model == 0 else rank2(h)


def final_model(model, Mn, T1, T2):
    """H21i = T2inv * Hn * T1 with H12i = its inverse, or F21i = T2^T * Fn * T1 (left to right)."""
    if model == 0:
        M = mul3(mul3(inverse3(T2), Mn), T1)
        return M, inverse3(M)
    return mul3(mul3(f32(T2).T, Mn), T1), np.zeros((3, 3), F)


def fix_sign(M):
    """The matrix with its largest-magnitude entry made positive."""
    m = f32(M).reshape(-1)
    return f32(M) if m[np.argmax(np.abs(m))] >= 0 else f32(-f32(M))


# ---------------------------------------------------------------------------------------------------- scoring
def _near(value, threshold):
    return np.abs(value.astype(np.float64) - float(threshold)) <= MARGIN * abs(float(threshold))


def _chain(t1, t2):
    """score += t1[0]; score += t2[0]; score += t1[1]; ... in float32."""
    terms = np.stack([t1, t2], 1).reshape(-1).astype(F)
    return np.add.accumulate(terms, dtype=F)[-1] if terms.shape[0] else F(0)


def check_homography(H21, H12, sigma, pt1, pt2):
    """-> (score, inliers [n] bool, borderline [n] bool)"""
    h, hi = f32(H21).reshape(9), f32(H12).reshape(9)
    u1, v1, u2, v2 = f32(pt1[:, 0]), f32(pt1[:, 1]), f32(pt2[:, 0]), f32(pt2[:, 1])
    th = F(5.991)
    inv_sigma2 = F(1.0 / float(F(F(sigma) * F(sigma))))
    with np.errstate(all="ignore"):
        w = f32(f32(f32(hi[6] * u2) + f32(hi[7] * v2)) + hi[8])
        winv = (1.0 / w.astype(np.float64)).astype(F)
        a = f32(f32(f32(f32(hi[0] * u2) + f32(hi[1] * v2)) + hi[2]) * winv)
        b = f32(f32(f32(f32(hi[3] * u2) + f32(hi[4] * v2)) + hi[5]) * winv)
        d1 = f32(f32(f32(u1 - a) * f32(u1 - a)) + f32(f32(v1 - b) * f32(v1 - b)))
        chi1 = f32(d1 * inv_sigma2)
        w = f32(f32(f32(h[6] * u1) + f32(h[7] * v1)) + h[8])
        winv = (1.0 / w.astype(np.float64)).astype(F)
        a = f32(f32(f32(f32(h[0] * u1) + f32(h[1] * v1)) + h[2]) * winv)
        b = f32(f32(f32(f32(h[3] * u1) + f32(h[4] * v1)) + h[5]) * winv)
        d2 = f32(f32(f32(u2 - a) * f32(u2 - a)) + f32(f32(v2 - b) * f32(v2 - b)))
        chi2 = f32(d2 * inv_sigma2)
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, F(0), f32(th - chi1)).astype(F)
        t2 = np.where(out2, F(0), f32(th - chi2)).astype(F)
    return _chain(t1, t2), ~(out1 | out2), _near(chi1, th) | _near(chi2, th)


def check_fundamental(F21, sigma, pt1, pt2):
    f = f32(F21).reshape(9)
    u1, v1, u2, v2 = f32(pt1[:, 0]), f32(pt1[:, 1]), f32(pt2[:, 0]), f32(pt2[:, 1])
    th, th_score = F(3.841), F(5.991)
    inv_sigma2 = F(1.0 / float(F(F(sigma) * F(sigma))))
    with np.errstate(all="ignore"):
        a2 = f32(f32(f32(f[0] * u1) + f32(f[1] * v1)) + f[2])
        b2 = f32(f32(f32(f[3] * u1) + f32(f[4] * v1)) + f[5])
        c2 = f32(f32(f32(f[6] * u1) + f32(f[7] * v1)) + f[8])
        num2 = f32(f32(f32(a2 * u2) + f32(b2 * v2)) + c2)
        chi1 = f32(f32(f32(num2 * num2) / f32(f32(a2 * a2) + f32(b2 * b2))) * inv_sigma2)
        a1 = f32(f32(f32(f[0] * u2) + f32(f[3] * v2)) + f[6])
        b1 = f32(f32(f32(f[1] * u2) + f32(f[4] * v2)) + f[7])
        c1 = f32(f32(f32(f[2] * u2) + f32(f[5] * v2)) + f[8])
        num1 = f32(f32(f32(a1 * u1) + f32(b1 * v1)) + c1)
        chi2 = f32(f32(f32(num1 * num1) / f32(f32(a1 * a1) + f32(b1 * b1))) * inv_sigma2)
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, F(0), f32(th_score - chi1)).astype(F)
        t2 = np.where(out2, F(0), f32(th_score - chi2)).astype(F)
    return _chain(t1, t2), ~(out1 | out2), _near(chi1, th) | _near(chi2, th)


def check(model, M, Minv, sigma, pt1, pt2):
    return check_homography(M, Minv, sigma, pt1, pt2) if model == 0 else check_fundamental(M, sigma, pt1, pt2)


def select(scores):
    """(best score, its iteration): the first with the strictly greatest score above 0; (0, -1) without one (:172,223)."""
    best, idx = F(0), -1
    for it, s in enumerate(f32(scores)):
        if s > best:
            best, idx = s, it
    return best, idx


def branch(sh, sf):
    """1: ReconstructH, 0: ReconstructF, -1: SH + SF == 0 (:113-128); and RH."""
    if F(F(sh) + F(sf)) == 0:
        return -1, F(0)
    rh = F(F(sh) / F(F(sh) + F(sf)))
    return (1 if float(rh) > 0.50 else 0), rh


# ---------------------------------------------------------------------------------------------------- CheckRT
def row_dot(Rrow, v):
    return sum3(f32(Rrow[0] * v[..., 0]), f32(Rrow[1] * v[..., 1]), f32(Rrow[2] * v[..., 2]))


def norm3(v):
    s = sum3(f32(v[..., 0] * v[..., 0]), f32(v[..., 1] * v[..., 1]), f32(v[..., 2] * v[..., 2]))
    return np.sqrt(s.astype(np.float64)).astype(F)


def parallax_of(cosines):
    """:890-898 from the cosines CheckRT kept."""
    if len(cosines) == 0:
        return F(0)
    c = np.sort(f32(cosines))[min(50, len(cosines) - 1)]
    with np.errstate(invalid="ignore"):
        a = F(np.arccos(np.float64(c)))          # NaN beyond 1, as acos in C
    return F(float(F(a * F(180))) / math.pi)


def check_rt(K, R, t, sigma, pt1, pt2, inliers, x3d=None):
    """CheckRT for one motion hypothesis -> dict(code [n]: 0 not counted, 1 counted, 2 counted and vbGood; x3d [n, 3]; cos [n];
    n_good; parallax; borderline [n]).  x3d: points to use in place of the triangulation (the build under test's), for the matches
    where it has any."""
    K, R, t = f32(K), f32(R).reshape(3, 3), f32(t)
    n = pt1.shape[0]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    P1 = np.concatenate([K, np.zeros((3, 1), F)], 1)
    Rt = np.concatenate([R, t.reshape(3, 1)], 1)
    P2 = np.zeros((3, 4), F)
    for i in range(3):
        for j in range(4):
            P2[i, j] = sum3(F(K[i, 0] * Rt[0, j]), F(K[i, 1] * Rt[1, j]), F(K[i, 2] * Rt[2, j]))
    O2 = np.array([sum3(F(-R[0, i] * t[0]), F(-R[1, i] * t[1]), F(-R[2, i] * t[2])) for i in range(3)], F)
    u1, v1, u2, v2 = f32(pt1[:, 0]), f32(pt1[:, 1]), f32(pt2[:, 0]), f32(pt2[:, 1])
    th2 = F(4.0 * float(F(F(sigma) * F(sigma))))
    with np.errstate(all="ignore"):
        A = np.stack([f32(u1[:, None] * P1[2]) - P1[0], f32(v1[:, None] * P1[2]) - P1[1],
                      f32(u2[:, None] * P2[2]) - P2[0], f32(v2[:, None] * P2[2]) - P2[1]], 1).astype(F)
        h = np.linalg.svd(A.astype(np.float64))[2][:, 3, :] if n else np.zeros((0, 4))
        p = (h[:, :3] / h[:, 3:4]).astype(F)
        if x3d is not None:
            have = np.asarray(x3d, F).any(axis=1)
            p[have] = np.asarray(x3d, F)[have]
        finite = np.isfinite(p).all(axis=1)
        dist1 = norm3(p)
        n2 = f32(p - O2)
        dist2 = norm3(n2)
        cosp = f32(sum3(f32(p[:, 0] * n2[:, 0]), f32(p[:, 1] * n2[:, 1]), f32(p[:, 2] * n2[:, 2])) / f32(dist1 * dist2))
        low = cosp.astype(np.float64) < 0.99998
        p2 = np.stack([f32(row_dot(R[i], p) + t[i]) for i in range(3)], 1)
        invz1 = (1.0 / p[:, 2].astype(np.float64)).astype(F)
        ex = f32(f32(f32(f32(fx * p[:, 0]) * invz1) + cx) - u1)
        ey = f32(f32(f32(f32(fy * p[:, 1]) * invz1) + cy) - v1)
        e1 = f32(f32(ex * ex) + f32(ey * ey))
        invz2 = (1.0 / p2[:, 2].astype(np.float64)).astype(F)
        ex = f32(f32(f32(f32(fx * p2[:, 0]) * invz2) + cx) - u2)
        ey = f32(f32(f32(f32(fy * p2[:, 1]) * invz2) + cy) - v2)
        e2 = f32(f32(ex * ex) + f32(ey * ey))
        counted = np.asarray(inliers, bool) & finite & ~((p[:, 2] <= 0) & low) & ~((p2[:, 2] <= 0) & low) & ~(e1 > th2) & ~(e2 > th2)
        scale = np.abs(p).max(axis=1) if n else np.zeros(0)
        borderline = (_near(cosp, 0.99998) | (np.abs(p[:, 2]) < MARGIN * scale) | (np.abs(p2[:, 2]) < MARGIN * scale) | _near(e1, th2) | _near(e2, th2))
    code = np.where(counted, np.where(low, 2, 1), 0).astype(np.uint8)
    return dict(code=code, x3d=np.where(counted[:, None], p, F(0)).astype(F), cos=cosp, n_good=int(counted.sum()),
                parallax=parallax_of(cosp[counted]), borderline=borderline & np.asarray(inliers, bool))


# ---------------------------------------------------------------------------------------------------- the decisions
def decide(branch_, N, n_good, parallax):
    """(status, winner) of ReconstructF (branch 0, four hypotheses) or ReconstructH (branch 1, eight)."""
    min_parallax, min_triangulated = F(1.0), 50
    if branch_ == 0:
        g = [int(x) for x in n_good[:4]]
        max_good = max(g)
        n_min_good = max(int(0.9 * N), min_triangulated)
        nsimilar = sum(1 for x in g if x > 0.7 * max_good)
        winner = g.index(max_good)
        if max_good < n_min_good:
            return capi.OSH_TWOVIEW_TOO_FEW_POINTS, winner
        if nsimilar > 1:
            return capi.OSH_TWOVIEW_NO_CLEAR_WINNER, winner
        return (capi.OSH_TWOVIEW_ACCEPTED_F if F(parallax[winner]) > min_parallax else capi.OSH_TWOVIEW_LOW_PARALLAX), winner
    best, second, idx, best_parallax = 0, 0, -1, F(-1)
    for i in range(8):
        if n_good[i] > best:
            second, best, idx, best_parallax = best, int(n_good[i]), i, F(parallax[i])
        elif n_good[i] > second:
            second = int(n_good[i])
    if not second < 0.75 * best:
        return capi.OSH_TWOVIEW_NO_CLEAR_WINNER, idx
    if not (best > min_triangulated and best > 0.9 * N):
        return capi.OSH_TWOVIEW_TOO_FEW_POINTS, idx
    if not best_parallax >= min_parallax:
        return capi.OSH_TWOVIEW_LOW_PARALLAX, idx
    return capi.OSH_TWOVIEW_ACCEPTED_H, idx


# ---------------------------------------------------------------------------------------------------- glibc rand()
def glibc_rand(seed, count):
    """The first `count` values of glibc's rand() after srand(seed) (TYPE_3: the additive feedback generator r[i] = r[i-3] + r[i-31])."""
    r = [0] * (344 + count)
    r[0] = seed if seed != 0 else 1
    for i in range(1, 31):
        hi, lo = divmod(r[i - 1], 127773)
        w = 16807 * lo - 2836 * hi
        r[i] = w + 2147483647 if w < 0 else w
    for i in range(31, 34):
        r[i] = r[i - 31]
    for i in range(34, 344 + count):
        r[i] = (r[i - 31] + r[i - 3]) & 0xFFFFFFFF
    return [x >> 1 for x in r[344:]]


def replay_sets(stream, n, iterations):
    """mvSets (:79-98) from a list of rand() values, consumed from the front: ([iterations, 8], values used)."""
    sets, k = np.zeros((iterations, 8), np.int32), 0
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            randi = int((stream[k] / (2147483647 + 1.0)) * len(avail))
            k += 1
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets, k


def truth_error(T21, R_true, t_true):
    """(rotation angle to the truth in degrees, angle between the translation directions in degrees)."""
    R, t = np.asarray(T21[:9], np.float64).reshape(3, 3), np.asarray(T21[9:], np.float64)
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R.T @ R_true) - 1) / 2))))
    c = float(t @ t_true) / (np.linalg.norm(t) * np.linalg.norm(t_true))
    return ang, math.degrees(math.acos(max(-1.0, min(1.0, c))))
