"""FP64 numpy restatement of the 4-DoF pose graph of Optimizer::OptimizeEssentialGraph4DoF, used by the tests only.

The algebra of csrc/pgo4_se3.h with the same operation order: ExpSO3 / LogSO3 / NormalizeRotation (src/G2oTypes.cc:782-813,
the polar factor by the same Newton iteration), ImuCamPose::UpdateW as VertexPose4DoF::oplusImpl drives it
(src/G2oTypes.cc:222-256), Edge4DoF::computeError (include/G2oTypes.h:817-845), the central-difference Jacobians of
base_binary_edge.hpp:147-196 on pushed copies of the vertex state, a direct sparse solve of H + lambda I, and the
Levenberg-Marquardt controller of optimization_algorithm_levenberg.cpp:99-184 with lambda_0 from computeLambdaInit.

A vertex state is a dict of arrays over a leading axis: DR, Rwb, Rcw [n, 3, 3], twb, tcw [n, 3], its [n]; the constants are
Rwb0 = the initial Rwb, Rcb, tcb.  Every function takes a dtype: np.float64 (the default, the device's precision) or
np.longdouble.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from pgo_numpy import require_extended  # noqa: F401  (re-exported for the tests)

TAU = 1e-5


def m3_mul(A, B):
    """A B, each entry summed left to right."""
    return A[..., :, 0:1] * B[..., 0:1, :] + A[..., :, 1:2] * B[..., 1:2, :] + A[..., :, 2:3] * B[..., 2:3, :]


def m3_mul_bt(A, B):
    return m3_mul(A, np.swapaxes(B, -1, -2))


def m3_vec(A, v):
    return A[..., :, 0] * v[..., 0:1] + A[..., :, 1] * v[..., 1:2] + A[..., :, 2] * v[..., 2:3]


def m3_tvec(A, v):
    return m3_vec(np.swapaxes(A, -1, -2), v)


def normalize_rotation(R, dtype=np.float64):
    R = np.array(R, dtype=dtype).reshape(-1, 3, 3)
    active = np.ones(len(R), bool)
    half = dtype(0.5)
    for _ in range(12):
        if not active.any():
            break
        A = R[active]
        r = A.reshape(-1, 9).T
        c00, c10, c20 = r[4] * r[8] - r[5] * r[7], r[5] * r[6] - r[3] * r[8], r[3] * r[7] - r[4] * r[6]
        idt = dtype(1) / (r[0] * c00 + r[1] * c10 + r[2] * c20)
        Ri = np.stack([c00 * idt, (r[2] * r[7] - r[1] * r[8]) * idt, (r[1] * r[5] - r[2] * r[4]) * idt,
                       c10 * idt, (r[0] * r[8] - r[2] * r[6]) * idt, (r[2] * r[3] - r[0] * r[5]) * idt,
                       c20 * idt, (r[1] * r[6] - r[0] * r[7]) * idt, (r[0] * r[4] - r[1] * r[3]) * idt], -1).reshape(-1, 3, 3)
        nv = half * (A + np.swapaxes(Ri, -1, -2))
        d = np.abs(nv - A).reshape(-1, 9).max(axis=1)
        R[active] = nv
        idx = np.flatnonzero(active)
        active[idx[d < 1e-16]] = False
    return R


def exp_so3(w, dtype=np.float64):
    w = np.asarray(w, dtype=dtype).reshape(-1, 3)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    d2 = x * x + y * y + z * z
    d = np.sqrt(d2)
    zero = np.zeros_like(x)
    W = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(-1, 3, 3)
    W2 = m3_mul(W, W)
    eye = np.eye(3, dtype=dtype)
    small = d < 1e-5
    R = np.empty_like(W)
    R[small] = (eye + W[small]) + dtype(0.5) * W2[small]
    big = ~small
    if big.any():
        db, d2b = d[big][:, None, None], d2[big][:, None, None]
        R[big] = (eye + (W[big] * np.sin(db)) / db) + (W2[big] * (dtype(1) - np.cos(db))) / d2b
    return normalize_rotation(R, dtype)


def log_so3(R, dtype=np.float64):
    R = np.asarray(R, dtype=dtype).reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    w = np.stack([(R[:, 2, 1] - R[:, 1, 2]) / 2, (R[:, 0, 2] - R[:, 2, 0]) / 2, (R[:, 1, 0] - R[:, 0, 1]) / 2], -1)
    c = (tr - dtype(1)) * dtype(0.5)
    ok = (c <= 1) & (c >= -1)
    theta = np.arccos(np.where(ok, c, 0))
    s = np.sin(theta)
    ok &= np.abs(s) >= 1e-5
    out = w.copy()
    out[ok] = (theta[ok][:, None] * w[ok]) / s[ok][:, None]
    return out


def initial_state(g, dtype=np.float64):
    n = len(g.fixed)
    return dict(DR=np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3)).copy(), Rwb=np.array(g.Rwb, dtype=dtype),
                twb=np.array(g.twb, dtype=dtype), Rcw=np.array(g.Rcw, dtype=dtype), tcw=np.array(g.tcw, dtype=dtype),
                its=np.zeros(n, np.int64))


def take(st, idx):
    return {k: v[idx] for k, v in st.items()}


def update_w(st, Rwb0, Rcb, tcb, u, dtype=np.float64):
    """UpdateW(0, 0, u0, u1, u2, u3) on copies: returns the new state."""
    u = np.asarray(u, dtype=dtype).reshape(-1, 4)
    zero = np.zeros(len(u), dtype=dtype)
    dR = exp_so3(np.stack([zero, zero, u[:, 0]], -1), dtype)
    DR = m3_mul(dR, st["DR"])
    Rwb = m3_mul(DR, np.asarray(Rwb0, dtype=dtype))
    twb = st["twb"] + u[:, 1:4]
    its = st["its"] + 1
    norm = its >= 5
    if norm.any():
        D = DR[norm]
        D[:, 0, 2] = 0.0
        D[:, 1, 2] = 0.0
        D[:, 2, 0] = 0.0
        D[:, 2, 1] = 0.0
        DR[norm] = normalize_rotation(D, dtype)
        its = np.where(norm, 0, its)
    Rbw = np.swapaxes(Rwb, -1, -2)
    tbw = -m3_vec(Rbw, twb)
    Rcb = np.asarray(Rcb, dtype=dtype)
    return dict(DR=DR, Rwb=Rwb, twb=twb, Rcw=m3_mul(Rcb, Rbw), tcw=m3_vec(Rcb, tbw) + np.asarray(tcb, dtype=dtype), its=its)


def edge_error(dR, dt, Rcwi, tcwi, Rcwj, tcwj, dtype=np.float64):
    B = m3_mul_bt(m3_mul_bt(np.asarray(Rcwi, dtype=dtype), np.asarray(Rcwj, dtype=dtype)), np.asarray(dR, dtype=dtype))
    er = log_so3(B, dtype)
    r = m3_vec(np.asarray(Rcwi, dtype=dtype), -m3_tvec(np.asarray(Rcwj, dtype=dtype), np.asarray(tcwj, dtype=dtype)))
    et = (r + np.asarray(tcwi, dtype=dtype)) - np.asarray(dt, dtype=dtype)
    return np.concatenate([er, et], -1)


def errors(g, st, dtype=np.float64):
    i, j = g.edge_ij[:, 0], g.edge_ij[:, 1]
    return edge_error(g.dR, g.dt, st["Rcw"][i], st["tcw"][i], st["Rcw"][j], st["tcw"][j], dtype)


def chi2_edges(g, e, dtype=np.float64):
    w = np.asarray(g.info_diag, dtype=dtype)
    c = np.zeros(len(e), dtype=dtype)
    for k in range(6):
        c = c + e[:, k] * (w[k] * e[:, k])
    return c


def jacobians(g, st, dtype=np.float64):
    """Numeric Jacobians [E, 6, 4] of both sides (zero for a fixed side), delta 1e-9, each evaluation on a pushed copy."""
    i, j = g.edge_ij[:, 0], g.edge_ij[:, 1]
    E = len(i)
    delta = dtype(1e-9)
    scalar = dtype(1) / (2 * delta)
    Ji = np.zeros((E, 6, 4), dtype=dtype)
    Jj = np.zeros((E, 6, 4), dtype=dtype)
    si, sj = take(st, i), take(st, j)
    for d in range(4):
        add = np.zeros((E, 4), dtype=dtype)
        add[:, d] = delta
        for side, (sv, v) in enumerate(((si, i), (sj, j))):
            ev = []
            for sgn in (add, -add):
                sp = update_w(sv, g.Rwb[v], g.Rcb[v], g.tcb[v], sgn, dtype)
                if side == 0:
                    ev.append(edge_error(g.dR, g.dt, sp["Rcw"], sp["tcw"], sj["Rcw"], sj["tcw"], dtype))
                else:
                    ev.append(edge_error(g.dR, g.dt, si["Rcw"], si["tcw"], sp["Rcw"], sp["tcw"], dtype))
            (Ji if side == 0 else Jj)[:, :, d] = scalar * (ev[0] - ev[1])
    Ji[g.fixed[i]] = 0
    Jj[g.fixed[j]] = 0
    return Ji, Jj


def _system(g, st, dtype=np.float64):
    free = np.flatnonzero(~g.fixed)
    sys = -np.ones(len(g.fixed), dtype=np.int64)
    sys[free] = np.arange(len(free))
    return free, sys


def linearize(g, st=None, dtype=np.float64):
    """chi2, H = J^T Omega J (dense, free vertices in array order) and b = -J^T Omega e."""
    st = initial_state(g, dtype) if st is None else st
    free, sys = _system(g, st, dtype)
    e = errors(g, st, dtype)
    Ji, Jj = jacobians(g, st, dtype)
    w = np.asarray(g.info_diag, dtype=dtype)
    N = 4 * len(free)
    H = np.zeros((N, N), dtype=dtype)
    b = np.zeros(N, dtype=dtype)
    for k, (vi, vj) in enumerate(g.edge_ij):
        Js = ((sys[vi], Ji[k]), (sys[vj], Jj[k]))
        for a, Ja in Js:
            if a < 0:
                continue
            b[4 * a:4 * a + 4] -= (Ja * w[:, None]).T @ e[k]
            for c, Jc in Js:
                if c < 0:
                    continue
                H[4 * a:4 * a + 4, 4 * c:4 * c + 4] += (Ja * w[:, None]).T @ Jc
    chi2 = np.sum(chi2_edges(g, e, dtype))
    return (float(chi2) if dtype == np.float64 else chi2), H, b


def _assemble_sparse(g, sys, Ji, Jj, e, N):
    import scipy.sparse as sp
    w = np.asarray(g.info_diag, dtype=np.float64)
    rows, cols, vals = [], [], []
    b = np.zeros(N)
    ii = np.arange(4)
    for side_a, Ja_all in ((0, Ji), (1, Jj)):
        a = sys[g.edge_ij[:, side_a]]
        m = a >= 0
        WJ = Ja_all[m] * w[None, :, None]
        np.add.at(b, (4 * a[m])[:, None] + ii, -np.einsum("ekr,ek->er", WJ, e[m]))
        for side_c, Jc_all in ((0, Ji), (1, Jj)):
            c = sys[g.edge_ij[:, side_c]]
            mm = m & (c >= 0)
            blk = np.einsum("ekr,ekc->erc", Ja_all[mm] * w[None, :, None], Jc_all[mm])
            rows.append(np.broadcast_to((4 * a[mm])[:, None, None] + ii[:, None], blk.shape).ravel())
            cols.append(np.broadcast_to((4 * c[mm])[:, None, None] + ii[None, :], blk.shape).ravel())
            vals.append(blk.ravel())
    H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    return H, b


@dataclass
class Pgo4Solution:
    state: dict
    iterations: int
    trials: int
    chi2_initial: float
    chi2_final: float
    lambda_init: float
    max_its_updates: int      # the most accepted updates of any one vertex


def optimize(g, iterations=20, lambda_init=0.0, trace=None) -> Pgo4Solution:
    """g2o's Levenberg-Marquardt; lambda_init = 0 takes computeLambdaInit (tau * max |diag H| of the free vertices)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    st = initial_state(g)
    free, sys = _system(g, st)
    N = 4 * len(free)
    lam, ni, n_bad = lambda_init, 2.0, 0
    its = trials = 0
    chi2_initial, lam0 = None, 0.0
    updates = np.zeros(len(g.fixed), np.int64)
    for it in range(iterations):
        e = errors(g, st)
        current = float(np.sum(chi2_edges(g, e)))
        if chi2_initial is None:
            chi2_initial = current
        ini = current
        Ji, Jj = jacobians(g, st)
        H, b = _assemble_sparse(g, sys, Ji, Jj, e, N)
        if it == 0:
            lam = lambda_init if lambda_init > 0 else TAU * float(np.max(np.abs(H.diagonal()), initial=0.0))
            lam0, ni, n_bad = lam, 2.0, 0
        q = 0
        rho = 0.0
        while True:
            A = (H + lam * sp.identity(N, format="csc")).tocsc()
            x = spla.spsolve(A, b)
            ok2 = bool(np.all(np.isfinite(x)))
            trial = {k: v.copy() for k, v in st.items()}
            up = update_w(take(st, free), g.Rwb[free], g.Rcb[free], g.tcb[free], x.reshape(-1, 4))
            for k in trial:
                trial[k][free] = up[k]
            et = errors(g, trial)
            temp = float(np.sum(chi2_edges(g, et))) if ok2 else np.finfo(np.float64).max
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
                st = trial
                updates[free] += 1
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
    e = errors(g, st)
    return Pgo4Solution(st, its, trials, chi2_initial if chi2_initial is not None else 0.0, float(np.sum(chi2_edges(g, e))), lam0,
                        int(updates.max(initial=0)))


def pack_state(st):
    """The device layout of a vertex state: [n, 34] = DR Rwb twb Rcw tcw its."""
    n = len(st["its"])
    return np.concatenate([st["DR"].reshape(n, 9), st["Rwb"].reshape(n, 9), st["twb"], st["Rcw"].reshape(n, 9), st["tcw"],
                           st["its"].astype(np.float64)[:, None]], 1).astype(np.float64)


def unpack_state(a):
    a = np.asarray(a).reshape(-1, 34)
    return dict(DR=a[:, 0:9].reshape(-1, 3, 3), Rwb=a[:, 9:18].reshape(-1, 3, 3), twb=a[:, 18:21], Rcw=a[:, 21:30].reshape(-1, 3, 3),
                tcw=a[:, 30:33], its=a[:, 33].astype(np.int64))
