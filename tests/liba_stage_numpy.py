"""References for the stage tests of the two inertial kernels (k_liba, k_posei).

noise_floor    how far the ORACLE's own stage outputs move when the float32 preintegration record of the problem is moved by one
               float32 ulp per entry.  The project explains the tolerances of its inertial comparisons with the float32 getters of
               that record (device and host libm differ by an ulp in sinf / cosf); this measures that explanation on the reference
               alone, so a bound derived from it owes nothing to the code under test.
measures       the distances the stage tests use (relative to the largest entry; H scaled by its diagonal).
trial_ld       one Levenberg-Marquardt trial in np.longdouble from given H, b, Hll, Hpl and lambda: the Schur complement, an
               iteratively refined solve (pgo_numpy.solve_ld) and the landmark back-substitution.
full_solve_ld  the same trial without the Schur route: one refined solve of the whole (keyframes + landmarks) system."""
import copy

import numpy as np

import pgo_numpy as pn

LD = np.longdouble
N_COPIES = 8
SEED = 20240229


# ---- measures -------------------------------------------------------------------------------------------------------
def rel_max(a, ref):
    """Largest entry of |a - ref| relative to the largest entry of |ref|."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    s = np.abs(ref).max() if ref.size else 0.0
    return float(np.abs(a - ref).max() / s) if s > 0 else float(np.abs(a - ref).max() if a.size else 0.0)


def scaled_h(a, ref):
    """Largest |dH_ij| / sqrt(H_ii H_jj) over the rows and columns whose diagonal entry is positive (the others must be equal)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    dg = np.diag(ref)
    ok = dg > 0
    d = np.abs(a - ref)
    assert np.all(d[~ok, :] == 0) and np.all(d[:, ~ok] == 0), "a row without a positive diagonal entry differs"
    if not ok.any():
        return 0.0
    s = np.sqrt(dg[ok])
    return float((d[np.ix_(ok, ok)] / np.outer(s, s)).max())


def rel_scalar(a, ref):
    return float(abs(float(a) - float(ref)) / abs(float(ref))) if float(ref) != 0 else float(abs(float(a)))


# ---- the reference's own noise ---------------------------------------------------------------------------------------
def perturbed(problem, field, k):
    """Copy k of `problem` with every entry of its float32 record `field` moved one float32 ulp up or down (fixed seed)."""
    rec = np.ascontiguousarray(getattr(problem, field), dtype=np.float32)
    rng = np.random.default_rng(SEED + k)
    up = rng.integers(0, 2, size=rec.shape).astype(bool)
    moved = np.where(up, np.nextafter(rec, np.float32(np.inf)), np.nextafter(rec, np.float32(-np.inf))).astype(np.float32)
    q = copy.copy(problem)
    setattr(q, field, np.ascontiguousarray(moved))
    return q


def noise_floor(fn, problem, field, measures=None):
    """fn(problem) -> {name: array or scalar} is an oracle stage function.  Returns {name: the largest distance of the outputs of
    N_COPIES one-ulp perturbations of problem.<field> from the unperturbed output}, each in measures[name] (default rel_max)."""
    measures = measures or {}
    base = fn(problem)
    out = {k: 0.0 for k in base}
    for k in range(N_COPIES):
        got = fn(perturbed(problem, field, k))
        for name in base:
            out[name] = max(out[name], measures.get(name, rel_max)(got[name], base[name]))
    return out


# ---- one trial in extended precision ---------------------------------------------------------------------------------
def _landmark_columns(n, n_opt, Hpl, edge_pose, edge_point, L):
    """W [L][n][3]: the keyframe-landmark blocks as columns of the full system (pose i = rows 6i .. 6i+5; a left + right pair of
    a rig gives two edges on one block: their Hpl are added)."""
    W = np.zeros((L, n, 3), dtype=LD)
    for e, (ip, j) in enumerate(zip(edge_pose, edge_point)):
        if ip < n_opt:
            W[j, 6 * ip:6 * ip + 6, :] += np.asarray(Hpl[e], dtype=LD)
    return W


def _landmark_blocks(n_opt, Hpl, edge_pose, edge_point, L, dtype=LD):
    """Per landmark {pose: its 6 x 3 block}, a rig's left + right pair added into one block."""
    blocks = [dict() for _ in range(L)]
    for e, (ip, j) in enumerate(zip(edge_pose, edge_point)):
        if ip < n_opt:
            B = np.asarray(Hpl[e], dtype=dtype)
            blocks[j][int(ip)] = blocks[j][int(ip)] + B if int(ip) in blocks[j] else B
    return blocks


def trial_ld(H, b, Hll, Hpl, edge_pose, edge_point, n_opt, lam, dtype=LD):
    """(S, bs, x, xl) of one trial, np.longdouble.  H [n][n] with n = 15 n_opt (the 6-dof poses first, then v bg ba), b [n + 3L],
    Hll [L][3][3], Hpl [E][6][3] in the order of edge_pose / edge_point (blocks of fixed keyframes are ignored).
    dtype=np.float64: the same trial as plain float64 numpy does it (np.linalg.solve), to have numpy's own distance beside the device's."""
    pn.require_extended()
    LD = dtype
    H = np.asarray(H, dtype=LD)
    n, L = H.shape[0], len(Hll)
    b = np.asarray(b, dtype=LD)
    lam = LD(lam)
    blocks = _landmark_blocks(n_opt, Hpl, edge_pose, edge_point, L, LD)
    S = H + lam * np.eye(n, dtype=LD)
    bs = b[:n].copy()
    Dinv = np.zeros((L, 3, 3), dtype=LD)
    I3 = np.eye(3, dtype=LD)
    for j in range(L):
        Dinv[j] = _inv3_ld(np.asarray(Hll[j], dtype=LD) + lam * I3, LD)
        bl = b[n + 3 * j:n + 3 * j + 3]
        for i, Bi in blocks[j].items():
            BD = Bi @ Dinv[j]
            bs[6 * i:6 * i + 6] -= BD @ bl
            for k, Bk in blocks[j].items():
                S[6 * i:6 * i + 6, 6 * k:6 * k + 6] -= BD @ Bk.T
    x = pn.solve_ld(S, bs) if dtype == np.longdouble else np.linalg.solve(S, bs)
    xl = np.zeros((L, 3), dtype=LD)
    for j in range(L):
        t = b[n + 3 * j:n + 3 * j + 3].copy()
        for i, Bi in blocks[j].items():
            t -= Bi.T @ x[6 * i:6 * i + 6]
        xl[j] = Dinv[j] @ t
    return S, bs, x, xl


def _inv3_ld(A, dtype=LD):
    """Inverse of a 3 x 3 matrix by cofactors (np.linalg has no extended-precision path)."""
    c = np.empty((3, 3), dtype=dtype)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            s = [k for k in range(3) if k != j]
            c[j, i] = (-1) ** (i + j) * (A[r[0], s[0]] * A[r[1], s[1]] - A[r[0], s[1]] * A[r[1], s[0]])
    det = A[0, 0] * c[0, 0] + A[0, 1] * c[1, 0] + A[0, 2] * c[2, 0]
    return c / det


def full_solve_ld(H, b, Hll, Hpl, edge_pose, edge_point, n_opt, lam):
    """(x, xl) from ONE refined solve of the whole damped system [[H + lam I, W], [W^T, Hll + lam I]] -- no Schur complement."""
    pn.require_extended()
    n, L = np.asarray(H).shape[0], len(Hll)
    W = _landmark_columns(n, n_opt, Hpl, edge_pose, edge_point, L)
    A = np.zeros((n + 3 * L, n + 3 * L), dtype=LD)
    A[:n, :n] = np.asarray(H, dtype=LD)
    for j in range(L):
        A[:n, n + 3 * j:n + 3 * j + 3] = W[j]
        A[n + 3 * j:n + 3 * j + 3, :n] = W[j].T
        A[n + 3 * j:n + 3 * j + 3, n + 3 * j:n + 3 * j + 3] = np.asarray(Hll[j], dtype=LD)
    A += LD(lam) * np.eye(n + 3 * L, dtype=LD)
    x = pn.solve_ld(A, np.asarray(b, dtype=LD))
    return x[:n], x[n:].reshape(L, 3)
