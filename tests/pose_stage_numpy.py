"""A plain restatement of the contract of k_pose_opt (csrc/pose_device.hip), generic in its floating-point type: run in np.float64 and in
np.longdouble it is the reference of tests/test_pose_stage_cpu.py and tests/test_gpu_pose_stages.py.

It is vectorised over the edges of a frame (no per-edge Python loop) and shares no code with oracle/pose_oracle.c or oracle/pose_numpy.py.
What the reference library computes in float32 stays float32 in every run: 1/z, bf and their unfused product in the stereo residual,
theta and psi of KannalaBrandt8::project (taken as correctly rounded), the chi2 and the thresholds of the classification.

`optimize(frame, dtype)` returns what the device returns plus a trace of every Levenberg-Marquardt iteration.
"""
from types import SimpleNamespace

import numpy as np

MONO, STEREO, BODY = 0, 1, 2
TAU = 1e-5                      # OptimizationAlgorithmLevenberg::_tau
MAX_TRIALS = 10                 # _maxTrialsAfterFailure
BIG = float(np.float32(3.0e38))  # a float32 threshold that no chi2 exceeds


def require_extended():
    """The reference needs 80-bit (or wider) long double: fail loudly, never skip, where it is missing."""
    eps = np.finfo(np.longdouble).eps
    assert eps < 1e-18, f"np.longdouble has eps {eps}: this platform has no extended precision for the reference"


# ------------------------------------------------------------------------------------------------------------- rotations
def normalize_rotation(q):
    """SE3Quat::normalizeRotation: w >= 0, unit norm."""
    q = -q if q[3] < 0 else q
    return q / np.sqrt((q * q).sum())


def quat_mul(a, b):
    """Hamilton product a * b, quaternions as x y z w."""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], dtype=a.dtype)


def quat_rotate(q, v):
    """q v q^-1 for v [...,3] in Eigen's form v + w uv + q x uv, uv = 2 q x v (the quaternion is used as it is, not normalised)."""
    u = q[:3]
    uv = 2 * np.cross(np.broadcast_to(u, v.shape), v)
    return v + q[3] * uv + np.cross(np.broadcast_to(u, v.shape), uv)


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=q.dtype)


def R_to_quat(R):
    """Eigen's Quaternion(Matrix3), its branches in its order."""
    T = R.dtype.type
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, dtype=R.dtype)
    if t > 0:
        t = np.sqrt(t + T(1))
        q[3] = t / 2
        t = T(0.5) / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
        return q
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + T(1))
    q[i] = t / 2
    t = T(0.5) / t
    q[3] = (R[k, j] - R[j, k]) * t
    q[j] = (R[j, i] + R[i, j]) * t
    q[k] = (R[k, i] + R[i, k]) * t
    return q


def skew(w):
    z = w.dtype.type(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=w.dtype)


def pose_oplus(x, qt):
    """VertexSE3Expmap::oplusImpl: exp(x) * T, x = (omega, upsilon); SE3Quat::exp with its small-angle branch R = I + W + W W."""
    T = qt.dtype.type
    w, u = x[:3], x[3:]
    theta = np.sqrt((w * w).sum())
    W = skew(w)
    W2 = W @ W
    I = np.eye(3, dtype=qt.dtype)
    if theta < T(0.00001):
        R = I + W + W2
        V = R
    else:
        a = np.sin(theta) / theta
        b = (1 - np.cos(theta)) / (theta * theta)
        c = (theta - np.sin(theta)) / (theta * theta * theta)
        R = I + a * W + b * W2
        V = I + b * W + c * W2
    eq = normalize_rotation(R_to_quat(R))
    et = V @ u
    q = normalize_rotation(quat_mul(eq, qt[:4]))
    t = et + quat_rotate(eq, qt[4:])
    return np.concatenate([q, t])


# ------------------------------------------------------------------------------------------------------------- cameras
def _f32(a):
    return np.asarray(a).astype(np.float32)


def kb8_project(fx, fy, cx, cy, kb, Xc, smooth=False):
    """KannalaBrandt8::project(Vector3d): theta and psi are float32 (correctly rounded atan2f / sqrtf of float32 arguments); `smooth`
    leaves them unrounded (the differentiable function that projectJac is the derivative of)."""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    r2 = x * x + y * y
    if smooth:
        theta, psi = np.arctan2(np.sqrt(r2), z), np.arctan2(y, x)
    else:
        root = _f32(np.sqrt(_f32(r2).astype(Xc.dtype))).astype(Xc.dtype)
        theta = _f32(np.arctan2(root, _f32(z).astype(Xc.dtype))).astype(Xc.dtype)
        psi = _f32(np.arctan2(_f32(y).astype(Xc.dtype), _f32(x).astype(Xc.dtype))).astype(Xc.dtype)
    t2 = theta * theta
    t3 = theta * t2
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    r = theta + kb[0] * t3 + kb[1] * t5 + kb[2] * t7 + kb[3] * t9
    return np.stack([fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy], axis=1)


def kb8_project_jac(fx, fy, kb, Xc):
    """KannalaBrandt8::projectJac: [E,2,3]."""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    x2, y2, z2 = x * x, y * y, z * z
    r2 = x2 + y2
    r = np.sqrt(r2)
    r3 = r2 * r
    th = np.arctan2(r, z)
    th2 = th * th
    th3, th4 = th2 * th, th2 * th2
    th5, th6, th8 = th4 * th, th2 * th4, th4 * th4
    th7, th9 = th6 * th, th8 * th
    f = th + th3 * kb[0] + th5 * kb[1] + th7 * kb[2] + th9 * kb[3]
    fd = 1 + 3 * kb[0] * th2 + 5 * kb[1] * th4 + 7 * kb[2] * th6 + 9 * kb[3] * th8
    den = r2 * (r2 + z2)
    J = np.zeros((Xc.shape[0], 2, 3), dtype=Xc.dtype)
    J[:, 0, 0] = fx * (fd * z * x2 / den + f * y2 / r3)
    J[:, 1, 0] = fy * (fd * z * y * x / den - f * y * x / r3)
    J[:, 0, 1] = fx * (fd * z * y * x / den - f * y * x / r3)
    J[:, 1, 1] = fy * (fd * z * y2 / den + f * x2 / r3)
    J[:, 0, 2] = -fx * fd * x / (r2 + z2)
    J[:, 1, 2] = -fy * fd * y / (r2 + z2)
    return J


def se3_deriv(Xc):
    """[0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1] for every point: [E,3,6]."""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    D = np.zeros((Xc.shape[0], 3, 6), dtype=Xc.dtype)
    D[:, 0, 1], D[:, 0, 2], D[:, 0, 3] = z, -y, 1
    D[:, 1, 0], D[:, 1, 2], D[:, 1, 4] = -z, x, 1
    D[:, 2, 0], D[:, 2, 1], D[:, 2, 5] = y, -x, 1
    return D


# ------------------------------------------------------------------------------------------------------------- the frame
class Problem:
    """The arrays of a synth.PoseFrame in the reference's type, split by edge kind once."""

    def __init__(self, f, dtype):
        self.T = T = np.dtype(dtype).type
        self.dtype = np.dtype(dtype)
        c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
        self.E = int(f.edge_kind.shape[0])
        self.X, self.obs, self.info = c(f.points).reshape(-1, 3), c(f.edge_obs).reshape(-1, 3), c(f.edge_info).reshape(-1)
        self.kind = np.asarray(f.edge_kind).astype(np.int64)
        self.cam = c(f.cam)
        self.kb8 = None if f.kb8 is None else c(f.kb8)
        self.cam2 = None if f.cam2 is None else c(f.cam2)
        self.trl = None if f.trl is None else c(f.trl)
        self.qt0 = c(f.pose_qt)
        self.delta = np.where(self.kind != STEREO, T(f.huber_mono), T(f.huber_stereo)).astype(dtype)
        self.th = np.stack([np.where(self.kind != STEREO, np.float32(f.chi2_mono[r]), np.float32(f.chi2_stereo[r])) for r in range(4)])
        self.budget = [int(k) for k in f.iterations]
        fish = self.kb8 is not None
        self.i_pin = np.flatnonzero((self.kind == MONO) & (not fish))
        self.i_kb8 = np.flatnonzero((self.kind == MONO) & fish)
        self.i_st = np.flatnonzero(self.kind == STEREO)
        self.i_body = np.flatnonzero(self.kind == BODY)
        assert not (fish and self.i_st.size), "a KannalaBrandt8 frame takes monocular and right-camera edges only"
        assert self.i_body.size == 0 or (fish and self.cam2 is not None and self.trl is not None)


def residuals(P, qt, smooth=False):
    """_error of every edge at pose qt: [E,3], row 2 zero for the two-row edges.  `smooth`: see kb8_project."""
    dt = P.dtype
    fx, fy, cx, cy = P.cam[0], P.cam[1], P.cam[2], P.cam[3]
    Xc = quat_rotate(qt[:4], P.X) + qt[4:]
    r = np.zeros((P.E, 3), dtype=dt)
    i = P.i_pin
    if i.size:
        r[i, 0] = P.obs[i, 0] - (fx * Xc[i, 0] / Xc[i, 2] + cx)
        r[i, 1] = P.obs[i, 1] - (fy * Xc[i, 1] / Xc[i, 2] + cy)
    i = P.i_st
    if i.size:
        invz32 = _f32(1 / Xc[i, 2])                       # const float invz = 1.0f / trans_xyz[2]
        bf32 = np.float32(P.cam[4])                       # const float& bf
        invz = invz32.astype(dt)
        u = Xc[i, 0] * invz * fx + cx
        v = Xc[i, 1] * invz * fy + cy
        bfz = (bf32 * invz32).astype(np.float32).astype(dt)   # float product
        r[i, 0], r[i, 1], r[i, 2] = P.obs[i, 0] - u, P.obs[i, 1] - v, P.obs[i, 2] - (u - bfz)
    i = P.i_kb8
    if i.size:
        r[i, :2] = P.obs[i, :2] - kb8_project(fx, fy, cx, cy, P.kb8, Xc[i], smooth)
    i = P.i_body
    if i.size:
        # (mTrl * T_lw).map(Xw): the SE3Quat product normalises its rotation
        q = normalize_rotation(quat_mul(P.trl[:4], qt[:4]))
        t = quat_rotate(P.trl[:4], qt[4:]) + P.trl[4:]
        Xr = quat_rotate(q, P.X[i]) + t
        c2 = P.cam2
        r[i, :2] = P.obs[i, :2] - kb8_project(c2[0], c2[1], c2[2], c2[3], c2[4:], Xr, smooth)
    return r, Xc


def jacobians(P, qt):
    """d _error / d (omega, upsilon) of every edge, the reference's analytic formulas term by term: [E,3,6]."""
    dt = P.dtype
    fx, fy, bf = P.cam[0], P.cam[1], P.cam[4]
    Xc = quat_rotate(qt[:4], P.X) + qt[4:]
    J = np.zeros((P.E, 3, 6), dtype=dt)
    i = P.i_pin
    if i.size:     # -Pinhole::projectJac * SE3deriv
        x, y, z = Xc[i, 0], Xc[i, 1], Xc[i, 2]
        pj = np.zeros((i.size, 2, 3), dtype=dt)
        pj[:, 0, 0], pj[:, 0, 2] = fx / z, -fx * x / (z * z)
        pj[:, 1, 1], pj[:, 1, 2] = fy / z, -fy * y / (z * z)
        J[i, :2] = np.einsum("eij,ejk->eik", -pj, se3_deriv(Xc[i]))
    i = P.i_st
    if i.size:     # EdgeStereoSE3ProjectXYZOnlyPose::linearizeOplus
        x, y = Xc[i, 0], Xc[i, 1]
        invz = 1 / Xc[i, 2]
        invz_2 = invz * invz
        Js = np.zeros((i.size, 3, 6), dtype=dt)
        Js[:, 0, 0] = x * y * invz_2 * fx
        Js[:, 0, 1] = -(1 + (x * x * invz_2)) * fx
        Js[:, 0, 2] = y * invz * fx
        Js[:, 0, 3] = -invz * fx
        Js[:, 0, 5] = x * invz_2 * fx
        Js[:, 1, 0] = (1 + y * y * invz_2) * fy
        Js[:, 1, 1] = -x * y * invz_2 * fy
        Js[:, 1, 2] = -x * invz * fy
        Js[:, 1, 4] = -invz * fy
        Js[:, 1, 5] = y * invz_2 * fy
        Js[:, 2, 0] = Js[:, 0, 0] - bf * y * invz_2
        Js[:, 2, 1] = Js[:, 0, 1] + bf * x * invz_2
        Js[:, 2, 2] = Js[:, 0, 2]
        Js[:, 2, 3] = Js[:, 0, 3]
        Js[:, 2, 5] = Js[:, 0, 5] - bf * invz_2
        J[i] = Js
    i = P.i_kb8
    if i.size:     # -KannalaBrandt8::projectJac * SE3deriv
        J[i, :2] = np.einsum("eij,ejk->eik", -kb8_project_jac(fx, fy, P.kb8, Xc[i]), se3_deriv(Xc[i]))
    i = P.i_body
    if i.size:     # -projectJac(X_r) * mTrl.rotation() * SE3deriv(X_l), X_r = mTrl.map(X_l)
        Xr = quat_rotate(P.trl[:4], Xc[i]) + P.trl[4:]
        pj = kb8_project_jac(P.cam2[0], P.cam2[1], P.cam2[4:], Xr)
        J[i, :2] = np.einsum("eij,jk,ekl->eil", -pj, quat_to_R(P.trl[:4]), se3_deriv(Xc[i]))
    return J


def chi2_of(P, r):
    w = P.info[:, None] * r
    return (r * w).sum(axis=1)


def huber(P, c):
    """RobustKernelHuber::robustify: rho and rho' of every edge's chi2."""
    d = P.delta
    inl = c <= d * d
    s = np.sqrt(np.where(inl, P.T(1), c))
    return np.where(inl, c, 2 * s * d - d * d), np.where(inl, P.T(1), d / s)


def build_system(P, qt, active, robust):
    """H = sum J^T (rho' Omega) J, b = sum J^T (-rho' Omega r) over the active edges, and their robust chi2."""
    r, _ = residuals(P, qt)
    c = chi2_of(P, r)
    rho0, rho1 = huber(P, c) if robust else (c, np.ones_like(c))
    J = jacobians(P, qt)
    a = active.astype(P.dtype)
    ww = rho1 * P.info * a
    H = np.einsum("eki,e,ekj->ij", J, ww, J)
    b = np.einsum("eki,ek->i", J, -(P.info * a * rho1)[:, None] * r)
    return H, b, (rho0 * a).sum()


def solve_ldlt(H, b, lam):
    """(H + lam I) x = b by an unpivoted LDL^T; fails unless every pivot is positive, and then x = 0."""
    n = b.shape[0]
    A = H.copy()
    A[np.diag_indices(n)] += lam
    L = np.eye(n, dtype=H.dtype)
    D = np.zeros(n, dtype=H.dtype)
    good = True
    for k in range(n):
        D[k] = A[k, k] - (L[k, :k] * L[k, :k] * D[:k]).sum()
        if not D[k] > 0:
            good = False
            break
        for i in range(k + 1, n):
            L[i, k] = (A[i, k] - (L[i, :k] * L[k, :k] * D[:k]).sum()) / D[k]
    if not good:
        return np.zeros(n, dtype=H.dtype), False
    y = b.copy()
    for k in range(n):
        y[k] = b[k] - (L[k, :k] * y[:k]).sum()
    y = y / D
    x = y.copy()
    for k in range(n - 1, -1, -1):
        x[k] = y[k] - (L[k + 1:, k] * x[k + 1:]).sum()
    return x, True


# ------------------------------------------------------------------------------------------------------------- the solver
def optimize(f, dtype=np.longdouble):
    """The four rounds of PoseOptimization on frame f.  Returns a namespace with the device's outputs (pose_qt, iterations, chi2_final,
    edge_chi2, outlier, n_bad, rounds), `evaluated` (edges whose chi2 was computed at least once: edge_chi2 of the others is undefined),
    `no_active` (per round: it met no active edge), `round_chi2` (per round: the chi2 its classification compared) and `trace`: per round a list with one dict per iteration: lam0 (lambda of its first trial), lams and rho (per trial), qmax, gain
    (ini - cur) / ini, nBad, chi (robust chi2 of the state it leaves), stop (None, "budget", "trials", "rho0", "nbad")."""
    P = Problem(f, dtype)
    T = P.T
    fmax = np.finfo(np.float64).max
    level = np.zeros(P.E, dtype=bool)
    chi2e = np.zeros(P.E, dtype=P.dtype)
    evaluated = np.zeros(P.E, dtype=bool)
    iterations, chi2_final = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=P.dtype)
    trace = [[] for _ in range(4)]
    round_chi2 = []                                        # every edge's chi2 as each round's classification saw it
    no_active = [False] * 4                                # rounds that met no active edge (optimize() returns at once)
    robust, n_bad, rounds = True, 0, 0
    qt_n = np.concatenate([normalize_rotation(P.qt0[:4]), P.qt0[4:]])
    qt = qt_n
    for rnd in range(4):
        qt = qt_n.copy()                                   # setEstimate(SE3Quat(q, t)) of every round
        active = ~level
        any_active = bool(active.any())
        no_active[rnd] = not any_active
        lam, ni, nBad, cj, last_chi, go = T(-1), T(2), 0, 0, T(0), True

        def evaluate(q):
            r, _ = residuals(P, q)
            c = chi2_of(P, r)
            chi2e[active] = c[active]
            evaluated[active] = True
            rho0 = huber(P, c)[0] if robust else c
            return rho0[active].sum()

        it = 0
        while it < P.budget[rnd] and go and any_active:
            H, b, _ = build_system(P, qt, active, robust)
            if it == 0:
                cur = evaluate(qt)                          # computeActiveErrors + activeRobustChi2 of the round's start
                lam, ni, nBad = T(TAU) * np.abs(np.diag(H)).max(), T(2), 0
            else:
                cur = last_chi                              # the accepted trial's sum
            ini = cur
            rec = dict(lam0=lam, lams=[], rho=[], qmax=0, stop=None)
            rho, qmax = T(0), 0
            while True:
                x, good = solve_ldlt(H, b, lam)
                trial = pose_oplus(x, qt)
                tmp = evaluate(trial)
                if not good:
                    tmp = T(fmax)
                scale = (x * (lam * x + b)).sum() + T(1e-3)   # computeScale
                with np.errstate(over="ignore"):            # a failed solve: (cur - DBL_MAX) / 1e-3 is -inf in float64
                    rho = (cur - tmp) / scale
                rec["lams"].append(lam)
                rec["rho"].append(rho)
                if rho > 0 and np.isfinite(tmp):
                    alpha = min(1 - (2 * rho - 1) ** 3, T(2) / T(3))
                    lam = lam * max(T(1) / T(3), alpha)
                    ni = T(2)
                    cur, qt = tmp, trial
                else:
                    lam = lam * ni
                    ni = ni * 2
                qmax += 1
                if not (rho < 0 and qmax < MAX_TRIALS):
                    break
            cj += 1
            it += 1
            last_chi = cur
            rec.update(qmax=qmax, chi=cur, gain=(ini - cur) / ini if ini != 0 else T(0))
            if qmax == MAX_TRIALS or rho == 0:
                go = False
                rec["stop"] = "trials" if qmax == MAX_TRIALS else "rho0"
            else:
                nBad = nBad + 1 if (ini - cur) * T(1e3) < ini else 0
                if nBad >= 3:
                    go = False
                    rec["stop"] = "nbad"
            if go and it == P.budget[rnd]:
                rec["stop"] = "budget"
            rec["nBad"] = nBad
            trace[rnd].append(rec)
        iterations[rnd], chi2_final[rnd] = cj, last_chi
        # classification: outliers of the previous round are re-evaluated at this round's final pose
        if level.any():
            r, _ = residuals(P, qt)
            c = chi2_of(P, r)
            chi2e[level] = c[level]
            evaluated[level] = True
        round_chi2.append(chi2e.copy())
        level = chi2e.astype(np.float32) > P.th[rnd]
        n_bad = int(level.sum())
        rounds = rnd + 1
        if rnd == 2:
            robust = False
        if P.E < 10:
            break
    return SimpleNamespace(pose_qt=qt, iterations=iterations, chi2_final=chi2_final, edge_chi2=chi2e, outlier=level.astype(np.uint8),
                           n_bad=n_bad, rounds=rounds, evaluated=evaluated, trace=trace, no_active=no_active,
                           round_chi2=round_chi2)
