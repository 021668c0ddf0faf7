"""FP64 numpy restatement of the Sim3 pose graph of Optimizer::OptimizeEssentialGraph, used by the tests only.

g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h: exp :70-146, map :144, log :148-231, inverse :233, product :266) vectorised over
a leading axis, EdgeSim3's error (types_seven_dof_expmap.h:99-112), the central-difference Jacobians of
base_binary_edge.hpp:147-196 through VertexSim3Expmap::oplusImpl (:60-69), a direct sparse solve of H + lambda I, and the
Levenberg-Marquardt controller of optimization_algorithm_levenberg.cpp:99-169 with this g2o copy's three-bad-iterations stop.
Sim3 arrays are [..., 8] = qx qy qz qw tx ty tz s.

Every Sim3 function, errors, jacobians and linearize take a dtype: np.float64 (the default, the precision of the device and of
g2o) or np.longdouble, the extended-precision reference the stage tests of the device compare both against.  Products,
inverses and maps follow the dtype of their inputs.  solve_ld solves a linear system to extended precision.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

EPS = 0.00001


def require_extended():
    """The reference needs 80-bit (or wider) long double: fail loudly, never skip, where it is missing."""
    eps = np.finfo(np.longdouble).eps
    assert eps < 1e-18, f"np.longdouble has eps {eps}: this platform has no extended precision for the reference"


def skew(w):
    z = np.zeros(w.shape[:-1], dtype=w.dtype)
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1),
                     np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def quat_to_R(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.stack([np.stack([1 - (tyy + tzz), txy - twz, txz + twy], -1),
                     np.stack([txy + twz, 1 - (txx + tzz), tyz - twx], -1),
                     np.stack([txz - twy, tyz + twx, 1 - (txx + tyy)], -1)], -2)


def R_to_quat(R, dtype=np.float64):
    """Eigen's Quaterniond(const Matrix3d&), no normalisation."""
    R = np.asarray(R, dtype=dtype)
    out = np.zeros(R.shape[:-2] + (4,), dtype=dtype)
    flatR = R.reshape(-1, 3, 3)
    flatq = out.reshape(-1, 4)
    for n in range(flatR.shape[0]):
        m = flatR[n]
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        q = flatq[n]
        if tr > 0:
            t = np.sqrt(tr + 1.0)
            q[3] = 0.5 * t
            t = 0.5 / t
            q[0] = (m[2, 1] - m[1, 2]) * t
            q[1] = (m[0, 2] - m[2, 0]) * t
            q[2] = (m[1, 0] - m[0, 1]) * t
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j, k = (i + 1) % 3, (i + 2) % 3
            t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
            q[i] = 0.5 * t
            t = 0.5 / t
            q[3] = (m[k, j] - m[j, k]) * t
            q[j] = (m[j, i] + m[i, j]) * t
            q[k] = (m[k, i] + m[i, k]) * t
    return out


def _R_to_quat_vec(R):
    """Vectorised R_to_quat for the trace > 0 case, falling back to the loop for the rest."""
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    q = np.zeros(R.shape[:-2] + (4,), dtype=R.dtype)
    pos = tr > 0
    with np.errstate(all="ignore"):
        t = np.sqrt(np.where(pos, tr, 0.0) + 1.0)
        w = 0.5 * t
        f = 0.5 / t
        q[..., 3] = w
        q[..., 0] = (R[..., 2, 1] - R[..., 1, 2]) * f
        q[..., 1] = (R[..., 0, 2] - R[..., 2, 0]) * f
        q[..., 2] = (R[..., 1, 0] - R[..., 0, 1]) * f
    if not np.all(pos):
        q[~pos] = R_to_quat(R[~pos], R.dtype)
    return q


def quat_rotate(q, v):
    vec = q[..., :3]
    uv = np.cross(vec, v)
    uv = uv + uv
    return v + q[..., 3:4] * uv + np.cross(vec, uv)


def quat_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def sim3_mul(a, b):
    q = quat_mul(a[..., :4], b[..., :4])
    t = a[..., 7:8] * quat_rotate(a[..., :4], b[..., 4:7]) + a[..., 4:7]
    return np.concatenate([q, t, (a[..., 7] * b[..., 7])[..., None]], -1)


def sim3_inverse(a):
    qc = np.concatenate([-a[..., :3], a[..., 3:4]], -1)
    t = quat_rotate(qc, (-1.0 / a[..., 7:8]) * a[..., 4:7])
    return np.concatenate([qc, t, (1.0 / a[..., 7])[..., None]], -1)


def sim3_map(a, p):
    return a[..., 7:8] * quat_rotate(a[..., :4], p) + a[..., 4:7]


def sim3_exp(u, dtype=np.float64):
    u = np.asarray(u, dtype=dtype)
    one = dtype(1)
    omega, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt(np.sum(omega * omega, -1))
    Om = skew(omega)
    Om2 = Om @ Om
    s = np.exp(sigma)
    I = np.eye(3, dtype=dtype)
    small_s = np.abs(sigma) < EPS
    small_t = theta < EPS
    with np.errstate(all="ignore"):
        th2 = theta * theta
        sg2 = sigma * sigma
        # |sigma| < eps
        A0 = np.where(small_t, 0.5, (1 - np.cos(theta)) / th2)
        B0 = np.where(small_t, one / 6, (theta - np.sin(theta)) / (th2 * theta))
        C1 = (s - 1) / sigma
        a = s * np.sin(theta)
        b = s * np.cos(theta)
        c = th2 + sg2
        A1 = np.where(small_t, ((sigma - 1) * s + 1) / sg2, (a * sigma + (1 - b) * theta) / (theta * c))
        B1 = np.where(small_t, ((0.5 * sg2 - sigma + 1) * s) / (sg2 * sigma), (C1 - ((b - 1) * sigma + a * theta) / c) * 1.0 / th2)
        A = np.where(small_s, A0, A1)
        B = np.where(small_s, B0, B1)
        C = np.where(small_s, 1.0, C1)
        f1 = np.where(small_t, 1.0, np.sin(theta) / theta)
        f2 = np.where(small_t, 1.0, (1 - np.cos(theta)) / th2)
    R = I + f1[..., None, None] * Om + f2[..., None, None] * Om2
    q = _R_to_quat_vec(R)
    W = A[..., None, None] * Om + B[..., None, None] * Om2 + C[..., None, None] * I
    t = np.einsum("...ij,...j->...i", W, ups)
    return np.concatenate([q, t, s[..., None]], -1)


def sim3_log(S, dtype=np.float64):
    S = np.asarray(S, dtype=dtype)
    one = dtype(1)
    s = S[..., 7]
    sigma = np.log(s)
    R = quat_to_R(S[..., :4])
    d = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    small_s = np.abs(sigma) < EPS
    small_d = d > 1 - EPS
    with np.errstate(all="ignore"):
        theta = np.arccos(np.where(small_d, 0.0, d))
        th2 = theta * theta
        f = np.where(small_d, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        omega = f[..., None] * dR
        sg2 = sigma * sigma
        A0 = np.where(small_d, 0.5, (1 - np.cos(theta)) / th2)
        B0 = np.where(small_d, one / 6, (theta - np.sin(theta)) / (th2 * theta))
        C1 = (s - 1) / sigma
        a = s * np.sin(theta)
        b = s * np.cos(theta)
        c = th2 + sg2
        A1 = np.where(small_d, ((sigma - 1) * s + 1) / sg2, (a * sigma + (1 - b) * theta) / (theta * c))
        B1 = np.where(small_d, ((0.5 * sg2 - sigma + 1) * s) / (sg2 * sigma), (C1 - ((b - 1) * sigma + a * theta) / c) * 1.0 / th2)
        A = np.where(small_s, A0, A1)
        B = np.where(small_s, B0, B1)
        C = np.where(small_s, 1.0, C1)
    Om = skew(omega)
    W = A[..., None, None] * Om + B[..., None, None] * (Om @ Om) + C[..., None, None] * np.eye(3, dtype=dtype)
    ups = _solve3_lu(W, S[..., 4:7], dtype)
    return np.concatenate([omega, ups, sigma[..., None]], -1)


def _solve3_lu(W, t, dtype=np.float64):
    """W.lu().solve(t) of every 3x3 system: partial pivoting by rows, elimination and back substitution in Eigen's order."""
    a = np.array(W, dtype=dtype, copy=True).reshape(-1, 3, 3)
    b = np.array(t, dtype=dtype, copy=True).reshape(-1, 3)
    r = np.arange(a.shape[0])
    for k in range(3):
        p = k + np.argmax(np.abs(a[:, k:, k]), axis=1)   # first maximum, as the strict > scan
        ak, ap = a[r, k].copy(), a[r, p].copy()
        a[r, k], a[r, p] = ap, ak
        bk, bp = b[r, k].copy(), b[r, p].copy()
        b[r, k], b[r, p] = bp, bk
        for i in range(k + 1, 3):
            l = a[:, i, k] / a[:, k, k]
            for c in range(k + 1, 3):
                a[:, i, c] -= l * a[:, k, c]
            b[:, i] -= l * b[:, k]
    x = np.zeros_like(b)
    for k in (2, 1, 0):
        s = b[:, k].copy()
        for c in range(k + 1, 3):
            s -= a[:, k, c] * x[:, c]
        x[:, k] = s / a[:, k, k]
    return x.reshape(np.shape(t))


def edge_error(meas, Si, Sj, dtype=np.float64):
    meas, Si, Sj = (np.asarray(a, dtype=dtype) for a in (meas, Si, Sj))
    return sim3_log(sim3_mul(sim3_mul(meas, Si), sim3_inverse(Sj)), dtype)


def oplus(est, upd, fix_scale, dtype=np.float64):
    upd = np.array(upd, dtype=dtype, copy=True)
    upd[..., 6] = np.where(fix_scale, 0.0, upd[..., 6])
    return sim3_mul(sim3_exp(upd, dtype), np.asarray(est, dtype=dtype))


@dataclass
class PgoGraph:
    estimate: np.ndarray      # [n, 8]
    fixed: np.ndarray         # [n] bool
    fix_scale: np.ndarray     # [n] bool
    edge_ij: np.ndarray       # [E, 2]
    measurement: np.ndarray   # [E, 8]


def errors(g: PgoGraph, est, dtype=np.float64):
    i, j = g.edge_ij[:, 0], g.edge_ij[:, 1]
    return edge_error(g.measurement, est[i], est[j], dtype)


def jacobians(g: PgoGraph, est, dtype=np.float64):
    """Numeric Jacobians [E, 7, 7] of both sides (zero for a fixed side), delta 1e-9, g2o's push / oplus / pop.  With
    np.longdouble the same central difference (the same float64 delta) is taken in extended precision."""
    i, j = g.edge_ij[:, 0], g.edge_ij[:, 1]
    E = len(i)
    est = np.asarray(est, dtype=dtype)
    delta = dtype(1e-9)
    scalar = dtype(1) / (2 * delta)
    Ji = np.zeros((E, 7, 7), dtype=dtype)
    Jj = np.zeros((E, 7, 7), dtype=dtype)
    for d in range(7):
        add = np.zeros((E, 7), dtype=dtype)
        add[:, d] = delta
        ep = edge_error(g.measurement, oplus(est[i], add, g.fix_scale[i], dtype), est[j], dtype)
        em = edge_error(g.measurement, oplus(est[i], -add, g.fix_scale[i], dtype), est[j], dtype)
        Ji[:, :, d] = scalar * (ep - em)
        ep = edge_error(g.measurement, est[i], oplus(est[j], add, g.fix_scale[j], dtype), dtype)
        em = edge_error(g.measurement, est[i], oplus(est[j], -add, g.fix_scale[j], dtype), dtype)
        Jj[:, :, d] = scalar * (ep - em)
    Ji[g.fixed[i]] = 0
    Jj[g.fixed[j]] = 0
    return Ji, Jj


def linearize(g: PgoGraph, est, dtype=np.float64):
    """chi2, H (dense, free vertices in array order) and b = -J^T e."""
    free = np.flatnonzero(~g.fixed)
    sys = -np.ones(len(g.fixed), dtype=np.int64)
    sys[free] = np.arange(len(free))
    e = errors(g, est, dtype)
    Ji, Jj = jacobians(g, est, dtype)
    N = 7 * len(free)
    H = np.zeros((N, N), dtype=dtype)
    b = np.zeros(N, dtype=dtype)
    for k, (vi, vj) in enumerate(g.edge_ij):
        Js = ((sys[vi], Ji[k]), (sys[vj], Jj[k]))
        for a, Ja in Js:
            if a < 0:
                continue
            b[7 * a:7 * a + 7] -= Ja.T @ e[k]
            for c, Jc in Js:
                if c < 0:
                    continue
                H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += Ja.T @ Jc
    chi2 = np.sum(e * e)
    return (float(chi2) if dtype == np.float64 else chi2), H, b


def solve_ld(A, b, sweeps=3):
    """x = A^-1 b to extended precision: an LU solve in float64, then iterative refinement with the residual b - A x computed
    in np.longdouble (A and b taken exactly as given).  Asserts that the refined residual is <= 1e-17 of |A| |x| + |b|
    (infinity norms), which needs kappa(A) well below 1 / 2^-53.  Returns x as np.longdouble."""
    import scipy.linalg as sla
    require_extended()
    A_ld, b_ld = np.asarray(A, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    lu = sla.lu_factor(np.asarray(A, dtype=np.float64))
    x = sla.lu_solve(lu, np.asarray(b, dtype=np.float64)).astype(np.longdouble)
    for _ in range(sweeps):
        r = b_ld - A_ld @ x
        x = x + sla.lu_solve(lu, r.astype(np.float64)).astype(np.longdouble)
    r = b_ld - A_ld @ x
    scale = np.abs(A_ld).sum(axis=1).max() * np.abs(x).max() + np.abs(b_ld).max()
    rel = np.abs(r).max() / scale if scale > 0 else np.longdouble(0)
    assert rel <= 1e-17, f"solve_ld: refined residual {float(rel):.3g} relative"
    return x


def _assemble_sparse(g, sys, Ji, Jj, e, N):
    import scipy.sparse as sp
    rows, cols, vals = [], [], []
    b = np.zeros(N)
    ii = np.arange(7)
    for side_a, Ja_all in ((0, Ji), (1, Jj)):
        a = sys[g.edge_ij[:, side_a]]
        m = a >= 0
        np.add.at(b, (7 * a[m])[:, None] + ii, -np.einsum("ekr,ek->er", Ja_all[m], e[m]))
        for side_c, Jc_all in ((0, Ji), (1, Jj)):
            c = sys[g.edge_ij[:, side_c]]
            mm = m & (c >= 0)
            blk = np.einsum("ekr,ekc->erc", Ja_all[mm], Jc_all[mm])
            rows.append(np.broadcast_to((7 * a[mm])[:, None, None] + ii[:, None], blk.shape).ravel())
            cols.append(np.broadcast_to((7 * c[mm])[:, None, None] + ii[None, :], blk.shape).ravel())
            vals.append(blk.ravel())
    H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    return H, b


@dataclass
class PgoSolution:
    estimate: np.ndarray
    iterations: int
    trials: int
    chi2_initial: float
    chi2_final: float


def optimize(g: PgoGraph, iterations=20, lambda_init=1e-16, trace=None, jacobian_dtype=np.float64) -> PgoSolution:
    """g2o's Levenberg-Marquardt; `trace`, a list, receives (iteration, rho, lambda of the trial, accepted) per trial.
    jacobian_dtype=np.longdouble takes the numeric Jacobians in extended precision (rounded to float64 for the solve): the
    distance between the two runs measures how far the Jacobians' float64 rounding alone moves the result."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    est = g.estimate.astype(np.float64).copy()
    free = np.flatnonzero(~g.fixed)
    sys = -np.ones(len(g.fixed), dtype=np.int64)
    sys[free] = np.arange(len(free))
    N = 7 * len(free)
    lam, ni, n_bad = lambda_init, 2.0, 0
    its = trials = 0
    chi2_initial = None
    for it in range(iterations):
        e = errors(g, est)
        current = float(np.sum(e * e))
        if chi2_initial is None:
            chi2_initial = current
        ini = current
        Ji, Jj = (J.astype(np.float64) for J in jacobians(g, est, jacobian_dtype))
        H, b = _assemble_sparse(g, sys, Ji, Jj, e, N)
        if it == 0:
            lam, ni, n_bad = lambda_init, 2.0, 0
        q = 0
        rho = 0.0
        while True:
            A = (H + lam * sp.identity(N, format="csc")).tocsc()
            x = spla.spsolve(A, b)
            ok2 = bool(np.all(np.isfinite(x)))
            trial = est.copy()
            trial[free] = oplus(est[free], x.reshape(-1, 7), g.fix_scale[free])
            et = errors(g, trial)
            temp = float(np.sum(et * et)) if ok2 else np.finfo(np.float64).max
            scale = float(np.dot(x, lam * x + b)) + 1e-3
            rho = (current - temp) / scale
            if trace is not None:
                trace.append((it, rho, lam, bool(rho > 0 and np.isfinite(temp))))
            if rho > 0 and np.isfinite(temp):
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current = temp
                est = trial
            else:
                lam *= ni
                ni *= 2
            q += 1
            trials += 1
            if not (rho < 0 and q < 10):
                break
        its += 1
        if q == 10 or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    e = errors(g, est)
    return PgoSolution(est, its, trials, chi2_initial if chi2_initial is not None else 0.0, float(np.sum(e * e)))
