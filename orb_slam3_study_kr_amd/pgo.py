"""Python driver over the Sim3 pose-graph C-ABI (include/orbslam3_hip.h, osh_pgo_*), and over the host layer's
Optimizer::OptimizeEssentialGraph on a stand-in map (include/orbslam3_hip_host.h, osh_host_pgo_*).

Thin plumbing only: every number of the solve is computed by the HIP kernels in csrc/pgo_device.hip.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi


@dataclass
class PgoGraph:
    """One Sim3 pose graph: Sim3 arrays are [.., 8] = qx qy qz qw tx ty tz s."""
    estimate: np.ndarray      # [n, 8] float64
    fixed: np.ndarray         # [n] bool
    fix_scale: np.ndarray     # [n] bool
    edge_ij: np.ndarray       # [E, 2] int32: vertex 0 (i), vertex 1 (j)
    measurement: np.ndarray   # [E, 8] float64 Sji

    def as_struct(self, iterations=20, lambda_init=1e-16, solve_mode=capi.OSH_PGO_SOLVE_ENVELOPE):
        self._keep = (np.ascontiguousarray(self.estimate, dtype=np.float64), np.ascontiguousarray(self.fixed, dtype=np.uint8),
                      np.ascontiguousarray(self.fix_scale, dtype=np.uint8), np.ascontiguousarray(self.edge_ij, dtype=np.int32).reshape(-1),
                      np.ascontiguousarray(self.measurement, dtype=np.float64).reshape(-1))
        est, fx, fs, eij, meas = self._keep
        return capi.PgoProblem(len(est), capi.ptr(est, capi.c_double_p), capi.ptr(fx, capi.c_uint8_p), capi.ptr(fs, capi.c_uint8_p),
                               len(eij) // 2, capi.ptr(eij, capi.c_int32_p), capi.ptr(meas, capi.c_double_p),
                               iterations, lambda_init, solve_mode)


@dataclass
class PgoResultArrays:
    estimate: np.ndarray
    iterations: int
    trials: int
    chi2_initial: float
    chi2_final: float
    envelope_entries: int
    envelope_tiles: int
    tall_columns: int


class PgoSolver:
    """Owns one ``osh_lba_ctx`` (one HIP device + stream) and runs pose graphs on it."""

    def __init__(self, device: int = 0):
        self.lib = capi.load_library()
        self.ctx = C.c_void_p()
        capi.check(self.lib.osh_lba_create(device, C.byref(self.ctx)), "osh_lba_create", self.lib)

    def close(self):
        if self.ctx:
            self.lib.osh_lba_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def solve(self, g: PgoGraph, iterations=20, lambda_init=1e-16, dense=False) -> PgoResultArrays:
        prob = g.as_struct(iterations, lambda_init, capi.OSH_PGO_SOLVE_DENSE if dense else capi.OSH_PGO_SOLVE_ENVELOPE)
        out = np.zeros((len(g.estimate), 8))
        res = capi.PgoResult()
        res.estimate = capi.ptr(out, capi.c_double_p)
        capi.check(self.lib.osh_pgo_solve(self.ctx, C.byref(prob), C.byref(res)), "osh_pgo_solve", self.lib)
        return PgoResultArrays(out, res.iterations, res.trials, res.chi2_initial, res.chi2_final, res.envelope_entries,
                               res.envelope_tiles, res.tall_columns)

    def linearize(self, g: PgoGraph):
        """chi2, H (dense, both triangles) and b = -J^T e of the first linearisation."""
        prob = g.as_struct()
        N = 7 * int(np.count_nonzero(~np.asarray(g.fixed, dtype=bool)))
        H = np.zeros((N, N))
        b = np.zeros(max(N, 1))
        chi2 = np.zeros(1)
        capi.check(self.lib.osh_pgo_linearize(self.ctx, C.byref(prob), capi.ptr(H, capi.c_double_p), capi.ptr(b, capi.c_double_p),
                                              capi.ptr(chi2, capi.c_double_p)), "osh_pgo_linearize", self.lib)
        return float(chi2[0]), H, b[:N]
