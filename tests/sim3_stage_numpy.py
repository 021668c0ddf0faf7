"""A restatement of the contract of k_sim3_opt (csrc/sim3opt_device.hip), generic in its floating-point type: run in np.float64 and in
np.longdouble it is the reference of tests/test_sim3_stage_cpu.py and tests/test_gpu_sim3_stages.py.

It states what tests/sim3opt_numpy.py states (the errors of EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ, g2o's central-difference
Jacobians of delta 1e-9 through VertexSim3Expmap::oplusImpl, Huber, buildSystem, the Levenberg-Marquardt controller, the two rounds and
both classifications) on pgo_numpy's g2o::Sim3 functions, which take a dtype, with the 7x7 solve in extended precision
(pgo_numpy.solve_ld) when the dtype is long double, and with the three budgets as arguments (osh_sim3_problem.iterations).

What the reference library computes in float32 stays float32 in every run: the threshold th2 and the Huber delta (float)sqrt(th2), and in
KannalaBrandt8::project the roundings of x^2 + y^2, of its square root, of Z, of theta and of psi (Y and X are rounded too).  kb8_project
returns those rounded values beside the pixel, so that two runs can be compared rounding by rounding.

A pack is the dict synth_sim3.pack() returns (X1c, X2c, obs1, obs2, info1, info2, cam1, cam2, kb8_1, kb8_2, S12, fix_scale, th2,
optionally iterations).  Sim3 arrays are qx qy qz qw tx ty tz s.
"""
from types import SimpleNamespace

import numpy as np

import pgo_numpy as pn

TAU = 1e-5                      # OptimizationAlgorithmLevenberg::_tau
MAX_TRIALS = 10                 # _maxTrialsAfterFailure
DELTA = 1e-9                    # the float64 delta of g2o's numeric Jacobian
BUDGETS = (5, 10, 5)            # optimize(5), optimize(nBad > 0 ? 10 : 5)
PLAIN_TH2 = float(np.float32(1e30))   # a th2 whose Huber delta no chi2 reaches: osh_sim3_linearize without kernels

require_extended = pn.require_extended


def _f32(a):
    return np.asarray(a).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- cameras
def kb8_project(cam, P):
    """KannalaBrandt8::project(Vector3d) of points P [..., 3]: (pixel [..., 2], roundings [..., 5] float32 = x2+y2, its root, Z, theta,
    psi).  The float32 arguments are exact in either dtype; atan2 and sqrt of them are taken as correctly rounded."""
    dt = P.dtype
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    r2 = _f32(X * X + Y * Y)
    root = _f32(np.sqrt(r2.astype(dt)))
    z32 = _f32(Z)
    theta32 = _f32(np.arctan2(root.astype(dt), z32.astype(dt)))
    psi32 = _f32(np.arctan2(_f32(Y).astype(dt), _f32(X).astype(dt)))
    theta, psi = theta32.astype(dt), psi32.astype(dt)
    t2 = theta * theta
    t3 = theta * t2
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    r = theta + cam[4] * t3 + cam[5] * t5 + cam[6] * t7 + cam[7] * t9
    uv = np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], -1)
    return uv, np.stack([r2, root, z32, theta32, psi32], -1)


def project(cam, kb8, P):
    """(pixel, roundings or None)."""
    if kb8:
        return kb8_project(cam, P)
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    return np.stack([cam[0] * X / Z + cam[2], cam[1] * Y / Z + cam[3]], -1), None


# ------------------------------------------------------------------------------------------------------------- the problem
class Problem:
    """The arrays of a pack in the reference's type."""

    def __init__(self, pk, dtype):
        self.dtype = np.dtype(dtype)
        self.T = T = self.dtype.type
        c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
        self.n = len(pk["info1"])
        self.X1c, self.X2c = c(pk["X1c"]).reshape(-1, 3), c(pk["X2c"]).reshape(-1, 3)
        self.obs1, self.obs2 = c(pk["obs1"]).reshape(-1, 2), c(pk["obs2"]).reshape(-1, 2)
        self.info1, self.info2 = c(pk["info1"]).reshape(-1), c(pk["info2"]).reshape(-1)
        self.cam1, self.cam2 = c(pk["cam1"]), c(pk["cam2"])
        self.kb8_1, self.kb8_2 = bool(pk["kb8_1"]), bool(pk["kb8_2"])
        self.S0 = c(pk["S12"])
        self.fix_scale = bool(pk["fix_scale"])
        th2 = np.float32(pk["th2"])
        self.th2 = T(th2)                                  # the float threshold, compared with the chi2 of the dtype
        self.delta = T(np.sqrt(th2))                       # const float deltaHuber = sqrt(th2)
        self.budgets = tuple(int(k) for k in pk.get("iterations", BUDGETS))


def oplus(P, S, x):
    return pn.oplus(S, x, P.fix_scale, P.T)


def errors(P, S, roundings=False):
    """(e12, e21) [..., n, 2] at estimate S [8] or at a stack of estimates [m, 8]; with `roundings` also the float32 roundings of the two
    projections (None for a Pinhole)."""
    Si = pn.sim3_inverse(S)
    if S.ndim == 2:
        S, Si = S[:, None, :], Si[:, None, :]
    u1, r1 = project(P.cam1, P.kb8_1, pn.sim3_map(S, P.X2c))
    u2, r2 = project(P.cam2, P.kb8_2, pn.sim3_map(Si, P.X1c))
    e12, e21 = P.obs1 - u1, P.obs2 - u2
    return (e12, e21, r1, r2) if roundings else (e12, e21)


def chi2(e, info):
    return e[..., 0] * (info * e[..., 0]) + e[..., 1] * (info * e[..., 1])


def huber(P, c, robust=True):
    """RobustKernelHuber::robustify: (rho, rho')."""
    if not robust:
        return c, np.ones_like(c)
    d = P.delta
    inl = c <= d * d
    s = np.sqrt(np.where(inl, P.T(1), c))
    return np.where(inl, c, 2 * s * d - d * d), np.where(inl, P.T(1), d / s)


def perturbed(P, S):
    """The 14 states Sim3(+-delta e_d) * S of the numeric Jacobian, rows +e0, -e0, +e1, ...: [14, 8]."""
    U = np.zeros((14, 7), dtype=P.dtype)
    for d in range(7):
        U[2 * d, d] = P.T(DELTA)
        U[2 * d + 1, d] = -P.T(DELTA)
    return oplus(P, S, U)


def jacobians(P, S, roundings=False):
    """J12, J21 [n, 2, 7]: (e(+delta) - e(-delta)) * (1 / (2 delta)), the inverse edge through the inverses of the perturbed states."""
    scalar = P.T(1) / (2 * P.T(DELTA))
    out = errors(P, perturbed(P, S), roundings)
    e12, e21 = out[0], out[1]
    J12 = np.transpose(scalar * (e12[0::2] - e12[1::2]), (1, 2, 0))
    J21 = np.transpose(scalar * (e21[0::2] - e21[1::2]), (1, 2, 0))
    return (J12, J21, out[2], out[3]) if roundings else (J12, J21)


def linearize(P, S, active, robust):
    """buildSystem over the active pairs: namespace(chi, H [7, 7], b [7], c12 [n], c21 [n], J12, J21, over12, over21), over* = the pair's
    edge is beyond the Huber threshold."""
    e12, e21 = errors(P, S)
    c12, c21 = chi2(e12, P.info1), chi2(e21, P.info2)
    J12, J21 = jacobians(P, S)
    a = active.astype(P.dtype)
    H = np.zeros((7, 7), dtype=P.dtype)
    b = np.zeros(7, dtype=P.dtype)
    chi = P.T(0)
    for e, c, J, info in ((e12, c12, J12, P.info1), (e21, c21, J21, P.info2)):
        r0, r1 = huber(P, c, robust)
        H = H + np.einsum("nra,n,nrc->ac", J, r1 * info * a, J)
        b = b + np.einsum("nra,nr->a", J, -(info * a * r1)[:, None] * e)
        chi = chi + (r0 * a).sum()
    d2 = P.delta * P.delta
    return SimpleNamespace(chi=chi, H=H, b=b, c12=c12, c21=c21, J12=J12, J21=J21, over12=c12 > d2, over21=c21 > d2)


def active_chi2(P, S, active, robust):
    e12, e21 = errors(P, S)
    c12, c21 = chi2(e12, P.info1), chi2(e21, P.info2)
    a = active.astype(P.dtype)
    return (huber(P, c12, robust)[0] * a).sum() + (huber(P, c21, robust)[0] * a).sum(), c12, c21


def solve(P, H, b, lam):
    """(H + lam I) x = b as LinearSolverDense: fails unless every pivot of the unpivoted LDL^T is positive, and then x = 0.  In long double
    the solution itself comes from pgo_numpy.solve_ld."""
    n = b.shape[0]
    A = H.copy()
    A[np.diag_indices(n)] += lam
    L = np.eye(n, dtype=H.dtype)
    D = np.zeros(n, dtype=H.dtype)
    for k in range(n):
        D[k] = A[k, k] - (L[k, :k] * L[k, :k] * D[:k]).sum()
        if not D[k] > 0:
            return np.zeros(n, dtype=H.dtype), False
        for i in range(k + 1, n):
            L[i, k] = (A[i, k] - (L[i, :k] * L[k, :k] * D[:k]).sum()) / D[k]
    if P.dtype == np.dtype(np.longdouble):
        return pn.solve_ld(A, b), True
    y = b.copy()
    for k in range(n):
        y[k] = b[k] - (L[k, :k] * y[:k]).sum()
    y = y / D
    x = y.copy()
    for k in range(n - 1, -1, -1):
        x[k] = y[k] - (L[k + 1:, k] * x[k + 1:]).sum()
    return x, True


def optimize(P, S, active, budget, robust, c12, c21):
    """initializeOptimization + optimize(budget) over the active pairs from S; c12 / c21 are overwritten for the active pairs by every
    evaluation.  Returns (S, iterations, chi2, trace): per iteration a dict lam0, lams, rho, ok (per trial), qmax, accepted (any trial),
    gain, nBad, chi, stop (None, "budget", "trials", "rho0", "nbad")."""
    T = P.T
    fmax = T(np.finfo(np.float64).max)
    lam, ni, nBad, cj, cur, go = T(0), T(2), 0, 0, T(0), True
    trace = []

    def keep(a12, a21):
        c12[active], c21[active] = a12[active], a21[active]

    it = 0
    while it < budget and go:
        L = linearize(P, S, active, robust)
        keep(L.c12, L.c21)
        cur = ini = L.chi
        if it == 0:
            lam, ni, nBad = T(TAU) * np.abs(np.diag(L.H)).max(), T(2), 0
        rec = dict(lam0=lam, lams=[], rho=[], ok=[], stop=None, S_in=S, H=L.H, b=L.b, x=[],
                   over=(int((L.over12 & active).sum() + (L.over21 & active).sum()), 2 * int(active.sum())))
        rho, qmax, accepted = T(0), 0, False
        while True:
            x, ok = solve(P, L.H, L.b, lam)
            if P.fix_scale:
                x[6] = 0
            trial = oplus(P, S, x)
            tmp, a12, a21 = active_chi2(P, trial, active, robust)
            keep(a12, a21)
            if not ok:
                tmp = fmax
            scale = (x * (lam * x + L.b)).sum() + T(1e-3)   # computeScale
            with np.errstate(over="ignore"):               # a failed solve: (cur - DBL_MAX) / 1e-3 is -inf in float64
                rho = (cur - tmp) / scale
            rec["lams"].append(lam); rec["rho"].append(rho); rec["ok"].append(ok); rec["x"].append(x)
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1 - (2 * rho - 1) ** 3, T(2) / T(3))
                lam = lam * max(T(1) / T(3), alpha)
                ni = T(2)
                cur, S, accepted = tmp, trial, True
            else:
                lam = lam * ni
                ni = ni * 2
            qmax += 1
            if not (rho < 0 and qmax < MAX_TRIALS):
                break
        cj += 1
        it += 1
        rec.update(qmax=qmax, accepted=accepted, chi=cur, gain=(ini - cur) / ini if ini != 0 else T(0))
        if qmax == MAX_TRIALS or rho == 0:
            go = False
            rec["stop"] = "trials" if qmax == MAX_TRIALS else "rho0"
        else:
            nBad = nBad + 1 if (ini - cur) * T(1e3) < ini else 0
            if nBad >= 3:
                go = False
                rec["stop"] = "nbad"
        if go and it == budget:
            rec["stop"] = "budget"
        rec["nBad"] = nBad
        trace.append(rec)
    return S, cj, cur, trace


def run(pk, dtype=np.longdouble, budgets=None):
    """Steps 1-5 of OptimizeSim3 on a pack with the budgets of the pack (or `budgets`).  Returns a namespace with the device's outputs
    (S12, outlier1, outlier, chi2_12, chi2_21, n_bad, n_in, round2, iterations, chi2_end) and S_round1 (the estimate round 1 left),
    chi2_round1 (both edges' chi2 as the round-1 classification saw them), budget2 (the round-2 budget taken), trace (per round),
    evaluated (pairs whose chi2 was computed at all) and at_S (pairs whose chi2 was last computed at the exported S12: the round-2
    inliers, and the round-1 outliers too when round 1 ended on an accepted trial and round 2 ran no iteration)."""
    P = Problem(pk, dtype)
    T = P.T
    bud = P.budgets if budgets is None else tuple(budgets)
    n = P.n
    c12, c21 = np.zeros(n, dtype=P.dtype), np.zeros(n, dtype=P.dtype)
    zero = np.zeros(n, np.uint8)
    res = SimpleNamespace(S12=P.S0, outlier1=zero, outlier=zero, chi2_12=c12, chi2_21=c21, n_bad=0, n_in=0, round2=False,
                          iterations=np.zeros(2, np.int64), chi2_end=np.zeros(2, dtype=P.dtype), S_round1=P.S0, chi2_round1=None,
                          trace=[[], []], budget2=None, evaluated=np.zeros(n, bool), at_S=np.zeros(n, bool))
    if n == 0:
        return res
    S1, it1, chi1, res.trace[0] = optimize(P, P.S0, np.ones(n, bool), bud[0], True, c12, c21)
    res.iterations[0], res.chi2_end[0], res.S_round1 = it1, chi1, S1
    res.chi2_round1 = (c12.copy(), c21.copy())
    res.evaluated = np.full(n, it1 > 0)
    out1 = (c12 > P.th2) | (c21 > P.th2)
    res.outlier1 = res.outlier = out1.astype(np.uint8)
    res.n_bad = int(out1.sum())
    if n - res.n_bad < 10:
        return res
    act = ~out1
    res.budget2 = bud[1] if res.n_bad > 0 else bud[2]
    S2, it2, chi2_, res.trace[1] = optimize(P, S1, act, res.budget2, False, c12, c21)
    res.iterations[1], res.chi2_end[1] = it2, chi2_
    e12, e21 = errors(P, S2)
    c12[act], c21[act] = chi2(e12, P.info1)[act], chi2(e21, P.info2)[act]
    fin = act & ((c12 > P.th2) | (c21 > P.th2))
    res.outlier = (out1 | fin).astype(np.uint8)
    res.n_in = int((act & ~fin).sum())
    res.round2, res.S12 = True, S2
    res.evaluated = np.ones(n, bool)
    res.at_S = act | bool(it1 > 0 and it2 == 0 and res.trace[0][-1]["accepted"])
    return res


def pair_chi2_at(pk, S, dtype=np.longdouble):
    """Both edges' chi2 of every pair at estimate S (given in any type, taken exactly)."""
    P = Problem(pk, dtype)
    e12, e21 = errors(P, np.asarray(S).astype(dtype))
    return chi2(e12, P.info1), chi2(e21, P.info2)


def first_linearization(pk, dtype=np.longdouble, robust=True):
    """osh_sim3_linearize: buildSystem at the input S12 over every pair (with th2 = PLAIN_TH2 for the plain one)."""
    if not robust:
        pk = dict(pk, th2=PLAIN_TH2)
    P = Problem(pk, dtype)
    return linearize(P, P.S0, np.ones(P.n, bool), True)


def linearization_roundings(pk, dtype):
    """The float32 roundings of both projections at the input S12 and at its 14 perturbed states: two arrays [15, n, 5] (None for a
    Pinhole)."""
    P = Problem(pk, dtype)
    states = np.concatenate([P.S0[None], perturbed(P, P.S0)])
    _, _, r1, r2 = errors(P, states, roundings=True)
    return r1, r2
