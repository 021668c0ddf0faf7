"""Extended-precision reference for the two dense LDL^T solvers of the reduced camera system (csrc/ldlt_block.h, csrc/big_solve.h).

The solvers read the upper triangle of S and b_s and return x.  `solve_refined` solves the same system in float64 and refines it
with residuals in np.longdouble until the residual stops shrinking (tests/pgo_numpy.py solve_ld does the same for the pose graph);
S and b_s are taken exactly as given.  For any candidate x (the device's, the oracle's):

    backward_error   eta(x) = |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf), evaluated in long double: how far x is from solving a nearby
                     system exactly.  A backward-stable factorisation gives a small multiple of 2^-53 whatever the conditioning.
    forward_error    eps(x) = |x - x_ref|_inf / |x_ref|_inf: grows with the condition number of S for every solver alike.

The solver tests hold the device to a multiple of what the oracle's own float64 no-pivot LDL^T reaches on the same system."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def require_extended():
    """The reference needs 80-bit (or wider) long double: fail loudly, never skip, where it is missing."""
    eps = np.finfo(LD).eps
    assert eps < 1e-18, f"np.longdouble has eps {eps}: this platform has no extended precision for the reference"


def symmetric(S):
    """The full symmetric matrix of a row-major S whose upper triangle is valid (the strict lower triangle is ignored)."""
    S = np.asarray(S, dtype=np.float64)
    U = np.triu(S)
    return U + np.triu(S, 1).T


def residual_norm(A_ld, x, b_ld):
    return float(np.abs(A_ld @ np.asarray(x, dtype=LD) - b_ld).max())


def solve_refined(S, b, max_sweeps=12):
    """(x_ref as np.longdouble, info) of the system (upper triangle of S, b): an LU solve in float64 and iterative refinement with
    long-double residuals until the residual stops shrinking.  info: A (symmetric float64), A_ld, b_ld, the residual norm after
    every sweep (`history`, the float64 solve first) and `converged` = the last residual is within 2^-60 of |A| |x| + |b|."""
    import scipy.linalg as sla
    require_extended()
    A = symmetric(S)
    A_ld, b_ld = A.astype(LD), np.asarray(b, dtype=LD)
    lu = sla.lu_factor(A)
    x = sla.lu_solve(lu, np.asarray(b, dtype=np.float64)).astype(LD)
    history = [residual_norm(A_ld, x, b_ld)]
    for _ in range(max_sweeps):
        r = b_ld - A_ld @ x
        cand = x + sla.lu_solve(lu, r.astype(np.float64)).astype(LD)
        rn = residual_norm(A_ld, cand, b_ld)
        if not rn < history[-1]:
            break
        x = cand
        history.append(rn)
    scale = float(np.abs(A_ld).sum(axis=1).max() * np.abs(x).max() + np.abs(b_ld).max())
    info = dict(A=A, A_ld=A_ld, b_ld=b_ld, history=history, scale=scale,
                converged=bool(history[-1] <= 2.0 ** -60 * scale) if scale > 0 else True)
    return x, info


def backward_error(info, x):
    """eta(x), normwise, in long double; `info` from solve_refined."""
    x = np.asarray(x, dtype=LD)
    r = np.abs(info["A_ld"] @ x - info["b_ld"]).max()
    den = np.abs(info["A_ld"]).sum(axis=1).max() * np.abs(x).max() + np.abs(info["b_ld"]).max()
    return float(r / den) if den > 0 else 0.0


def forward_error(x, x_ref):
    x_ref = np.asarray(x_ref, dtype=LD)
    den = np.abs(x_ref).max()
    return float(np.abs(np.asarray(x, dtype=LD) - x_ref).max() / den) if den > 0 else float(np.abs(np.asarray(x, dtype=LD)).max())


def errors(info, x_ref, x):
    return backward_error(info, x), forward_error(x, x_ref)
