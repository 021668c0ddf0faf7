"""Sim3 pose graphs and tangent vectors for the stage tests of the pose graph (test_pgo_cpu.py, test_gpu_pgo_stages.py),
built directly rather than through synth_pgo.make_map, plus a Python restatement of the solver's envelope bookkeeping."""
from __future__ import annotations

import numpy as np

import pgo_numpy as pn

LD = np.longdouble
EPS = pn.EPS


def _axis(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def branch_table():
    """Tangent vectors (omega, upsilon, sigma) whose Sim3 falls in each branch of g2o's exp and log, away from the thresholds.

    Returns a list of (name, u) with u a float64 [7].  exp branches on theta < 1e-5 and |sigma| < 1e-5, log on
    d = (tr R - 1) / 2 > 1 - 1e-5 (theta below ~4.47e-3) and |sigma| < 1e-5; theta runs up to 3.0 (not within 1e-3 of pi),
    the scale down to 0.05 and up to 20."""
    rng = np.random.default_rng(7)
    out = []
    # 8e-3 and 5e-5 sit in the large branches but within a factor 10 of the thresholds (a threshold moved to 1e-4 shows).
    # g2o's small-angle B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 (no "- 1": it does not tend to the true limit) grows as
    # 1 / sigma^3, so sigma = 5e-5 is paired only with angles whose central differences stay out of that branch.
    for th in (0.0, 1e-7, 2e-3, 8e-3, 0.5, 2.0, 3.0):
        for sg in (0.0, 3e-6, -4e-6, 5e-5, np.log(0.05), np.log(20.0), 0.3):
            if sg == 5e-5 and th < 5e-3:
                continue
            ups = rng.normal(size=3) * (0.5 if th < 1 else 2.0)
            out.append((f"th{th:g}_s{np.exp(sg):.6g}", np.concatenate([_axis(rng) * th, ups, [sg]])))
    return out


def near_threshold_table():
    """Tangent vectors within ~1e-8 (but not within rounding) of a branch threshold of log: |sigma| = 1e-5 (1 +- 1e-7), and
    theta with d = 1 - 1e-5 (1 +- 1e-6).  g2o's central difference (delta 1e-9) straddles the threshold there."""
    rng = np.random.default_rng(8)
    th_d = float(np.arccos(1 - EPS))    # d = cos(theta) for a pure rotation
    out = []
    for sg in (EPS * (1 + 1e-7), EPS * (1 - 1e-7), -EPS * (1 + 1e-7)):
        out.append((f"sigma_edge{sg:.9g}", np.concatenate([_axis(rng) * 0.4, rng.normal(size=3), [sg]])))
    for th in (th_d * (1 + 1e-6), th_d * (1 - 1e-6)):
        out.append((f"theta_edge{th:.9g}", np.concatenate([_axis(rng) * th, rng.normal(size=3), [0.2]])))
    return out


def random_sim3(rng, n, t_scale=3.0, s_range=(0.5, 2.0)):
    """[n, 8] float64 Sim3 with unit quaternions (w > 0 not enforced), translations ~ t_scale and log-uniform scales."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.normal(size=(n, 3)) * t_scale
    s = np.exp(rng.uniform(np.log(s_range[0]), np.log(s_range[1]), size=n))
    return np.concatenate([q, t, s[:, None]], 1)


def measurement_for(target_u, Si, Sj):
    """Sji with log(Sji * Si * Sj^-1) = target_u: exp(target_u) * Sj * Si^-1 in long double, rounded to float64."""
    T = pn.sim3_exp(np.asarray(target_u, LD), LD)
    Si, Sj = np.asarray(Si, LD), np.asarray(Sj, LD)
    return pn.sim3_mul(pn.sim3_mul(T, Sj), pn.sim3_inverse(Si)).astype(np.float64)


def make_graph(n, edges, fixed=(0,), fix_scale=False, seed=0, noise=1e-3, drift=0.05, t_scale=3.0):
    """A graph on n vertices with the given (i, j) edges: random true Sim3 poses, measurements = true relative pose with seeded
    noise, estimates = truth perturbed by `drift` (radians / units / log-scale).  fix_scale: bool or [n] bools."""
    rng = np.random.default_rng(seed)
    truth = random_sim3(rng, n, t_scale)
    fx = np.zeros(n, dtype=bool)
    fx[list(fixed)] = True
    fs = np.broadcast_to(np.asarray(fix_scale, dtype=bool), (n,)).copy()
    truth[fs, 7] = 1.0
    eij = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    meas = np.zeros((len(eij), 8))
    for k, (i, j) in enumerate(eij):
        u = rng.normal(size=7) * noise
        if fs[i] and fs[j]:
            u[6] = 0.0
        meas[k] = measurement_for(u, truth[i], truth[j])
    est = truth.copy()
    upd = rng.normal(size=(n, 7)) * drift
    upd[fx] = 0.0
    est[~fx] = pn.oplus(truth[~fx], upd[~fx], fs[~fx])
    return pn.PgoGraph(est, fx, fs, eij, meas)


def envelope_stats(g, dense=False, T=32):
    """The solver's envelope bookkeeping (pgo_device.hip make_plan) recomputed from edge_ij alone: (tiles, entries, tall)."""
    sys = -np.ones(len(g.fixed), dtype=np.int64)
    free = np.flatnonzero(~np.asarray(g.fixed, dtype=bool))
    sys[free] = np.arange(len(free))
    nf = len(free)
    minnb = np.arange(nf)
    for i, j in np.asarray(g.edge_ij).reshape(-1, 2):
        a, b = sys[i], sys[j]
        if a >= 0 and b >= 0 and a != b:
            lo, hi = min(a, b), max(a, b)
            minnb[hi] = min(minnb[hi], lo)
    N = 7 * nf
    NT = max(1, -(-N // T))
    entries = int(sum(49 * (a - minnb[a]) + 28 for a in range(nf)))
    tall = int(sum(1 for a in range(nf) if 7 * (a - minnb[a]) > 64))
    tiles = 0
    for J in range(NT):
        top = 0 if dense else min([J] + [(7 * minnb[c // 7]) // T for c in range(T * J, min(N, T * J + T))])
        tiles += J - top + 1
    return tiles, entries, tall


def block_errors(M, ref, nf):
    """Per 7x7 block (M: H [7nf, 7nf]) or per 7-vector (M: b [7nf]) relative error max|M - ref| / max|ref| over the non-zero
    blocks of ref; returns a flat array."""
    M, ref = np.asarray(M, LD), np.asarray(ref, LD)
    out = []
    if M.ndim == 1:
        for a in range(nf):
            r = ref[7 * a:7 * a + 7]
            sc = np.abs(r).max()
            if sc > 0:
                out.append(float(np.abs(M[7 * a:7 * a + 7] - r).max() / sc))
        return np.array(out)
    for a in range(nf):
        for c in range(a, nf):
            r = ref[7 * a:7 * a + 7, 7 * c:7 * c + 7]
            sc = np.abs(r).max()
            if sc > 0:
                out.append(float(np.abs(M[7 * a:7 * a + 7, 7 * c:7 * c + 7] - r).max() / sc))
    return np.array(out)
