"""A numpy FP64 restatement of MLPnPsolver (src/MLPnPsolver.cpp) for the tests of csrc/mlpnp.h and osh_orb_mlpnp_solve: computePose
with np.linalg for the SVDs, the eigenvectors and the solve, the Gauss-Newton (in any float type, so that it can be rerun in
np.longdouble), CheckInliers in float32, SetRansacParameters, and the record / Refine bookkeeping of iterate.  The Jacobian is the
analytic one; test_mlpnp_cpu.py checks it against central differences."""
from __future__ import annotations

import numpy as np

F = np.float32
EPS = np.finfo(np.float64).eps


def nullspace(f):
    """Columns 1 and 2 of V of the SVD of f^T (:371-373)."""
    _, _, vt = np.linalg.svd(np.asarray(f, np.float64).reshape(1, 3))
    return vt.T[:, 1:3]


def projector(f):
    f = np.asarray(f, np.float64)
    return np.eye(3) - np.outer(f, f) / (f @ f)


def rank3(S) -> int:
    """FullPivHouseholderQR::rank() restated with column pivoting: pivots above 3 * eps * the largest."""
    A = np.array(S, np.float64)
    d = []
    for k in range(3):
        norms = np.linalg.norm(A[k:, k:], axis=0)
        j = k + int(np.argmax(norms))
        A[:, [k, j]] = A[:, [j, k]]
        x = A[k:, k].copy()
        nx = np.linalg.norm(x)
        d.append(nx)
        if k < 2 and nx > 0:
            v = x.copy()
            v[0] += np.copysign(nx, x[0])
            v /= np.linalg.norm(v)
            A[k:, k:] -= 2 * np.outer(v, v @ A[k:, k:])
    d = np.array(d)
    return int(np.sum(d > 3 * EPS * d.max()))


def null_vector(M):
    return np.linalg.svd(np.asarray(M, np.float64))[2][-1]


def rodrigues2rot(w):
    w = np.asarray(w)
    dt = w.dtype
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)
    a = np.sqrt(w @ w)
    R = np.eye(3, dtype=dt)
    if a > EPS:
        R = R + np.sin(a) / a * W + (1 - np.cos(a)) / (a * a) * (W @ W)
    return R


def left_jacobian(w):
    w = np.asarray(w)
    dt = w.dtype
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)
    a = np.sqrt(w @ w)
    J = np.eye(3, dtype=dt)
    if a > EPS:
        J = J + (1 - np.cos(a)) / (a * a) * W + (a - np.sin(a)) / (a * a * a) * (W @ W)
    return J


def rot2rodrigues(R):
    with np.errstate(invalid="ignore"):
        wnorm = np.arccos((np.trace(R) - 1.0) / 2.0)
    omega = np.zeros(3)
    if wnorm > EPS:
        omega = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wnorm / (2.0 * np.sin(wnorm)))
    return omega


def residuals(x, pts, Ns):
    """r [n, 2] = N^T normalize(R(w) X + t)."""
    y = pts @ rodrigues2rot(x[:3]).T + x[3:]
    u = y / np.sqrt(np.sum(y * y, 1))[:, None]
    return np.einsum("nrc,nr->nc", Ns, u)


def residuals_and_jacs(x, pts, Ns):
    """r [n, 2] and J [n, 2, 6], the analytic derivative with respect to (omega, t)."""
    dt = x.dtype
    R, Jl = rodrigues2rot(x[:3]), left_jacobian(x[:3])
    Rp = pts @ R.T
    y = Rp + x[3:]
    ny = np.sqrt(np.sum(y * y, 1))
    u = y / ny[:, None]
    Pm = (np.eye(3, dtype=dt)[None] - u[:, :, None] * u[:, None, :]) / ny[:, None, None]
    C = np.zeros((pts.shape[0], 3, 3), dt)
    C[:, 0, 1], C[:, 0, 2], C[:, 1, 0], C[:, 1, 2], C[:, 2, 0], C[:, 2, 1] = -Rp[:, 2], Rp[:, 1], Rp[:, 2], -Rp[:, 0], -Rp[:, 1], Rp[:, 0]
    D = np.concatenate([-(Pm @ C @ Jl), Pm], 2)           # [n, 3, 6]
    return np.einsum("nrc,nr->nc", Ns, u), np.einsum("nrc,nra->nca", Ns, D)


def solve6(A, g):
    if A.dtype == np.float64:
        return np.linalg.solve(A, g)
    A, g = A.copy(), g.copy()   # Gaussian elimination with partial pivoting in the array's own float type
    n = g.shape[0]
    for k in range(n):
        j = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, j]], g[[k, j]] = A[[j, k]], g[[j, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            A[i, k:] -= m * A[k, k:]
            g[i] -= m * g[k]
    x = np.zeros(n, A.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (g[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def gauss_newton(x, pts, Ns, max_iterations: int = 5, dtype=np.float64):
    """mlpnp_gn (:694-758): (x, updates applied, how it ended: 0 its bound, 1 the break on dx, 2 the stop on J dx)."""
    x, pts, Ns = np.asarray(x, dtype).copy(), np.asarray(pts, dtype), np.asarray(Ns, dtype)
    updates = 0
    for _ in range(max_iterations):
        r, J = residuals_and_jacs(x, pts, Ns)
        Jm, rv = J.reshape(-1, 6), r.reshape(-1)
        try:
            dx = solve6(Jm.T @ Jm, Jm.T @ rv)
        except np.linalg.LinAlgError:
            dx = np.full(6, np.nan, dtype)
        a = np.abs(dx)
        if not np.isnan(a).any() and (a.max() > 5.0 or a.min() > 1.0):
            return x, updates, 1
        dl = np.abs(Jm @ dx)
        x = x - dx
        updates += 1
        if np.all(dl < 1e-5):
            return x, updates, 2
    return x, updates, 0


def compute_pose(f, p, eig_sign=(1, 1, 1), gn_dtype=np.float64, stages: dict = None):
    """computePose (:356-658) over all n >= 6 correspondences f, p [n, 3]: pose [12] = R row-major, t.  eig_sign: signs applied to
    the eigenvectors of the planar branch (they are free).  stages (a dict): gets planar, h, R0, t0, x0, updates, reason."""
    f, p = np.asarray(f, np.float64), np.asarray(p, np.float64)
    n = f.shape[0]
    Ns = np.stack([nullspace(v) for v in f])
    S = p.T @ p
    planar = rank3(S) == 2
    E = np.eye(3)
    pts = p
    if planar:
        _, vecs = np.linalg.eigh(S)
        E = (vecs * np.asarray(eig_sign, np.float64)[None, :]).T
        pts = p @ E.T
    ph = np.concatenate([pts, np.ones((n, 1))], 1)
    # column (r, a) of the row of correspondence i and null-space column c: N_i[r, c] * ph_i[a]
    cols = [(r, a) for r in range(3) for a in range(3)] + [(r, 3) for r in range(3)]
    if planar:
        cols = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (0, 3), (1, 3), (2, 3)]
    A = np.stack([(Ns[:, r, :] * ph[:, a, None]).reshape(-1) for r, a in cols], 1)
    h = null_vector(A.T @ A)
    if planar:
        tmp = np.array([[0, h[0], h[1]], [0, h[2], h[3]], [0, h[4], h[5]]])
        tmp[:, 0] = np.cross(tmp[:, 1], tmp[:, 2])
        tmp = tmp.T
        scale = 1.0 / np.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
        U, _, Vt = np.linalg.svd(tmp)
        R1 = U @ Vt
        if np.linalg.det(R1) < 0:
            R1 = -R1
        R1 = E.T @ R1
        t = scale * h[6:9]
        R1 = -R1.T
        if np.linalg.det(R1) < 0:
            R1[:, 2] *= -1
        R2 = R1 * np.array([-1.0, -1.0, 1.0])[None, :]
        cands = [(R1, t), (R1, -t), (R2, t), (R2, -t)]
        vals = []
        for Rc, tc in cands:
            y = p[:6] @ Rc.T + tc
            y = y / np.linalg.norm(y, axis=1)[:, None]
            vals.append(np.sum(1.0 - np.sum(y * f[:6], 1)))
        R0, t0 = cands[int(np.argmin(vals))]
    else:
        tmp = np.array([[h[0], h[3], h[6]], [h[1], h[4], h[7]], [h[2], h[5], h[8]]])
        scale = 1.0 / abs(np.linalg.norm(tmp[:, 0]) * np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])) ** (1.0 / 3.0)
        U, _, Vt = np.linalg.svd(tmp)
        Rp = U @ Vt
        if np.linalg.det(Rp) < 0:
            Rp = -Rp
        tp = Rp @ (scale * h[9:12])
        errs, Ts = [], []
        for sg in (1.0, -1.0):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = Rp, sg * tp
            T = np.linalg.inv(T)
            y = p[:6] @ T[:3, :3].T + T[:3, 3]
            y = y / np.linalg.norm(y, axis=1)[:, None]
            errs.append(np.sum(1.0 - np.sum(y * f[:6], 1)))
            Ts.append(T)
        t0 = Ts[0][:3, 3] if errs[0] < errs[1] else Ts[1][:3, 3]
        R0 = Ts[0][:3, :3]
    x0 = np.concatenate([rot2rodrigues(R0), t0])
    x, updates, reason = gauss_newton(x0, p, Ns, 5, gn_dtype)
    if stages is not None:
        stages.update(planar=planar, h=h, R0=R0, t0=t0, x0=x0, updates=updates, reason=reason, Ns=Ns)
    x = np.asarray(x, np.float64)
    return np.concatenate([rodrigues2rot(x[:3]).reshape(9), x[3:]])


def check_inliers(camera_type: int, cam, pose, p3d, p2d, max_error, with_error: bool = False):
    """CheckInliers (:262-293) in float32: the flags [n] (and error2)."""
    cam = np.asarray(cam, F)
    T = np.asarray(pose, np.float64)
    P = np.asarray(p3d, np.float64).astype(F).astype(np.float64)
    with np.errstate(all="ignore"):
        xc = (T[0] * P[:, 0] + T[1] * P[:, 1] + T[2] * P[:, 2] + T[9]).astype(F)
        yc = (T[3] * P[:, 0] + T[4] * P[:, 1] + T[5] * P[:, 2] + T[10]).astype(F)
        zc = (T[6] * P[:, 0] + T[7] * P[:, 1] + T[8] * P[:, 2] + T[11]).astype(F)
        if camera_type == 0:
            u = cam[0] * xc / zc + cam[2]
            v = cam[1] * yc / zc + cam[3]
        else:
            x2y2 = xc * xc + yc * yc
            theta = np.arctan2(np.sqrt(x2y2.astype(np.float64)).astype(F).astype(np.float64), zc.astype(np.float64)).astype(F)
            psi = np.arctan2(yc.astype(np.float64), xc.astype(np.float64)).astype(F)
            t2 = theta * theta
            t3 = theta * t2
            t5 = t3 * t2
            t7 = t5 * t2
            t9 = t7 * t2
            r = theta + cam[4] * t3 + cam[5] * t5 + cam[6] * t7 + cam[7] * t9
            u = cam[0] * r * np.cos(psi.astype(np.float64)).astype(F) + cam[2]
            v = cam[1] * r * np.sin(psi.astype(np.float64)).astype(F) + cam[3]
        p2d = np.asarray(p2d, F)
        dx, dy = p2d[:, 0] - u, p2d[:, 1] - v
        e2 = dx * dx + dy * dy
        flags = e2 < np.asarray(max_error, F)
    return (flags, e2) if with_error else flags


def ransac_parameters(N: int, probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5, th2=5.991):
    """SetRansacParameters (:225-260): (mRansacMinInliers, mRansacMaxIts)."""
    eps = F(epsilon)
    n_min = int(F(N) * eps)
    n_min = max(n_min, min_inliers, min_set)
    if N > 0 and eps < F(n_min) / F(N):
        eps = F(n_min) / F(N)
    if n_min == N:
        its = 1
    else:
        with np.errstate(all="ignore"):
            v = np.log(1 - probability) / np.log(1 - float(eps) ** 3)
        its = int(np.ceil(v)) if np.isfinite(v) else -(2 ** 31)
    return n_min, max(1, min(its, max_iterations))


def replay(count, min_inliers, best_in, ok_in, record_count):
    """The record scan and the decision of iterate (:169-222) as csrc/mlpnp.h states them: (records, dict)."""
    best, records = best_in, []
    for k, c in enumerate(count):
        if c >= min_inliers and c > best:
            best = c
            records.append(k)
    best, ok, rec, hit = best_in, int(bool(ok_in)), -1, -1
    for k, c in enumerate(count):
        if c >= min_inliers:
            if c > best:
                best, rec = c, rec + 1
                ok = int(record_count[rec] > min_inliers)
            if ok:
                hit = k
                break
    return records, dict(first_hit=hit, hit_record=rec if hit >= 0 else -1, hit_count=record_count[rec] if hit >= 0 and rec >= 0 else 0,
                         best_iteration=records[rec] if rec >= 0 else -1, best_count=best, best_refine_ok=ok, n_records=len(records))


def pose_difference(a, b):
    """(rotation angle in rad between the two rotations, norm of the translation difference)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dR = a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T
    s = np.linalg.norm(np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])) / 2.0
    return float(np.arcsin(min(1.0, s))), float(np.linalg.norm(a[9:] - b[9:]))
