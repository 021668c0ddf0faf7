"""FP64 numpy restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:2279-2385), used by the tests only.

Built on pgo_numpy's g2o::Sim3 functions: the errors of EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ through a Pinhole or a
KannalaBrandt8 (theta and psi rounded to float32 with the correctly rounded atan2 / sqrt convention of the device's atan2f_rn),
g2o's central-difference Jacobians (delta 1e-9) through VertexSim3Expmap::oplusImpl, Huber kernels of delta (float)sqrt(th2),
the Levenberg-Marquardt controller of optimization_algorithm_levenberg.cpp:99-169 with a dense 7x7 solve, and the two rounds,
classifications and early return of OptimizeSim3.  A pack is the dict synth_sim3.pack() returns.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import pgo_numpy as pn

DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def project(cam, kb8, P):
    """project(const Eigen::Vector3d&) of points P [..., 3]."""
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    if not kb8:
        return np.stack([cam[0] * X / Z + cam[2], cam[1] * Y / Z + cam[3]], -1)
    x2y2 = X * X + Y * Y
    sq = np.sqrt(_f32(x2y2).astype(np.float64)).astype(np.float32)
    theta = np.arctan2(sq.astype(np.float64), _f32(Z).astype(np.float64)).astype(np.float32).astype(np.float64)
    psi = np.arctan2(_f32(Y).astype(np.float64), _f32(X).astype(np.float64)).astype(np.float32).astype(np.float64)
    t2 = theta * theta
    t3 = theta * t2
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    r = theta + cam[4] * t3 + cam[5] * t5 + cam[6] * t7 + cam[7] * t9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], -1)


def errors(pk, S):
    """(e12 [n, 2], e21 [n, 2]) at estimate S (or at a stack of estimates S [m, 8] -> [m, n, 2])."""
    S = np.asarray(S, np.float64)
    Si = pn.sim3_inverse(S)
    if S.ndim == 2:
        S, Si = S[:, None, :], Si[:, None, :]
    e12 = pk["obs1"] - project(pk["cam1"], pk["kb8_1"], pn.sim3_map(S, pk["X2c"]))
    e21 = pk["obs2"] - project(pk["cam2"], pk["kb8_2"], pn.sim3_map(Si, pk["X1c"]))
    return e12, e21


def chi2(e, info):
    return e[..., 0] * (info * e[..., 0]) + e[..., 1] * (info * e[..., 1])


def huber(c, delta):
    """RobustKernelHuber::robustify: (rho0, rho1)."""
    d2 = delta * delta
    s = np.sqrt(c)
    big = c > d2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(big, 2 * s * delta - d2, c), np.where(big, delta / s, 1.0)


def perturbed(S, fix_scale):
    """The 14 states Sim3(+-delta e_d) * S of the numeric Jacobian: [14, 8], rows +e0, -e0, +e1, ..."""
    U = np.zeros((14, 7))
    for d in range(7):
        U[2 * d, d] = DELTA
        U[2 * d + 1, d] = -DELTA
    return np.stack([pn.oplus(S, U[k], fix_scale) for k in range(14)])


def jacobians(pk, S, delta=None):
    """J12, J21 [n, 2, 7]: g2o's recipe (delta 1e-9, (e+ - e-) * 1/(2 delta)); another delta gives a plain central difference."""
    if delta is None:
        P = perturbed(S, pk["fix_scale"])
        scalar = SCALAR
    else:
        U = np.zeros((14, 7))
        for d in range(7):
            U[2 * d, d] = delta
            U[2 * d + 1, d] = -delta
        P = np.stack([pn.oplus(S, U[k], pk["fix_scale"]) for k in range(14)])
        scalar = 1.0 / (2 * delta)
    e12, e21 = errors(pk, P)                     # [14, n, 2]
    J12 = scalar * (e12[0::2] - e12[1::2])       # [7, n, 2]
    J21 = scalar * (e21[0::2] - e21[1::2])
    return np.transpose(J12, (1, 2, 0)), np.transpose(J21, (1, 2, 0))


def linearize(pk, S, active, robust):
    """buildSystem over the active pairs: (robust chi2, H [7, 7], b [7], chi2_12 [n], chi2_21 [n])."""
    delta = float(np.float32(math.sqrt(np.float32(pk["th2"]))))
    e12, e21 = errors(pk, S)
    c12, c21 = chi2(e12, pk["info1"]), chi2(e21, pk["info2"])
    J12, J21 = jacobians(pk, S)
    H = np.zeros((7, 7))
    b = np.zeros(7)
    tot = []
    for e, c, J, info in ((e12, c12, J12, pk["info1"]), (e21, c21, J21, pk["info2"])):
        r0, r1 = huber(c, delta) if robust else (c, np.ones_like(c))
        w = (r1 * info)[active]
        Ja = J[active]
        H += np.einsum("n,nra,nrc->ac", w, Ja, Ja)
        wr = -(info[:, None] * e) * r1[:, None]
        b += np.einsum("nra,nr->a", Ja, wr[active])
        tot.append(r0[active])
    chi = math.fsum(np.concatenate(tot).tolist())
    return chi, H, b, c12, c21


def active_chi2(pk, S, active, robust):
    delta = float(np.float32(math.sqrt(np.float32(pk["th2"]))))
    e12, e21 = errors(pk, S)
    c12, c21 = chi2(e12, pk["info1"]), chi2(e21, pk["info2"])
    if robust:
        v = np.concatenate([huber(c12, delta)[0][active], huber(c21, delta)[0][active]])
    else:
        v = np.concatenate([c12[active], c21[active]])
    return math.fsum(v.tolist()), c12, c21


def _solve(H, lam, b):
    A = H + lam * np.eye(7)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


@dataclass
class RoundResult:
    S: np.ndarray
    iterations: int
    chi2: float
    c12: np.ndarray
    c21: np.ndarray
    last_gain: float = 0.0   # (iniChi - currentChi) / iniChi of the last iteration (the 1e-3 stop rule)


def optimize(pk, S, active, iterations, robust) -> RoundResult:
    """initializeOptimization + optimize(iterations) over the active pairs from S."""
    S = np.asarray(S, np.float64).copy()
    lam, ni, nbad, cj = 0.0, 2.0, 0, 0
    c12 = c21 = None
    cur = 0.0
    gain = 0.0
    for it in range(iterations):
        cur, H, b, c12, c21 = linearize(pk, S, active, robust)
        ini = cur
        if it == 0:
            lam = 1e-5 * np.max(np.abs(np.diag(H)))
            ni, nbad = 2.0, 0
        qmax, rho = 0, 0.0
        while True:
            x = _solve(H, lam, b)
            ok = x is not None
            if not ok:
                x = np.zeros(7)
            if pk["fix_scale"]:
                x[6] = 0.0
            St = pn.oplus(S, x, pk["fix_scale"])
            temp, c12, c21 = active_chi2(pk, St, active, robust)
            if not ok:
                temp = np.finfo(np.float64).max
            rho = (cur - temp) / (float(x @ (lam * x + b)) + 1e-3)
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = temp
                S = St
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        cj += 1
        if qmax == 10 or rho == 0:
            break
        gain = (ini - cur) / ini if ini else 0.0
        if (ini - cur) * 1e3 < ini:
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            break
    return RoundResult(S=S, iterations=cj, chi2=cur, c12=c12, c21=c21, last_gain=gain)


@dataclass
class Sim3Run:
    S12: np.ndarray
    outlier1: np.ndarray
    outlier: np.ndarray
    chi2_12: np.ndarray
    chi2_21: np.ndarray
    n_bad: int
    n_in: int
    round2: bool
    iterations: tuple
    chi2_end: tuple
    rounds: tuple


def run(pk) -> Sim3Run:
    """Steps 1-5 of OptimizeSim3 on a pack."""
    n = len(pk["index"])
    th2 = float(np.float32(pk["th2"]))
    S0 = np.asarray(pk["S12"], np.float64)
    out1 = np.zeros(n, np.uint8)
    if n == 0:
        return Sim3Run(S0, out1, out1.copy(), np.zeros(0), np.zeros(0), 0, 0, False, (0, 0), (0.0, 0.0), ())
    r1 = optimize(pk, S0, np.ones(n, bool), 5, True)
    out1 = ((r1.c12 > th2) | (r1.c21 > th2)).astype(np.uint8)
    n_bad = int(out1.sum())
    if n - n_bad < 10:
        return Sim3Run(S0, out1, out1.copy(), r1.c12, r1.c21, n_bad, 0, False, (r1.iterations, 0), (r1.chi2, 0.0), (r1,))
    act = out1 == 0
    r2 = optimize(pk, r1.S, act, 10 if n_bad > 0 else 5, False)
    e12, e21 = errors(pk, r2.S)
    c12 = np.where(act, chi2(e12, pk["info1"]), r1.c12)
    c21 = np.where(act, chi2(e21, pk["info2"]), r1.c21)
    fin = act & ((c12 > th2) | (c21 > th2))
    outlier = (out1.astype(bool) | fin).astype(np.uint8)
    n_in = int((act & ~fin).sum())
    return Sim3Run(r2.S, out1, outlier, c12, c21, n_bad, n_in, True, (r1.iterations, r2.iterations), (r1.chi2, r2.chi2), (r1, r2))


def classify(pk, S, active):
    """The final classification at a given estimate over the active pairs: (outlier flags, n_in)."""
    th2 = float(np.float32(pk["th2"]))
    e12, e21 = errors(pk, S)
    bad = (chi2(e12, pk["info1"]) > th2) | (chi2(e21, pk["info2"]) > th2)
    return active & bad, int((active & ~bad).sum())
