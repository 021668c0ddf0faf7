"""Python driver over the pose-graph C-ABI (include/orbslam3_hip.h: the Sim3 graph osh_pgo_*, the 4-DoF graph osh_pgo4_*),
and over the host layer's Optimizer::OptimizeEssentialGraph on a stand-in map (include/orbslam3_hip_host.h, osh_host_pgo_*).

Thin plumbing only: every number of the solve is computed by the HIP kernels in csrc/pgo_device.hip and csrc/pgo4_device.hip.
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


INFO_4DOF = (1e3, 1e3, 1.0, 1.0, 1.0, 1.0)   # OptimizeEssentialGraph4DoF's matLambda: (0, 0) set twice, (2, 2) never


@dataclass
class Pgo4Graph:
    """One 4-DoF pose graph (osh_pgo4_problem): 3x3 matrices are [.., 3, 3] float64."""
    Rwb: np.ndarray           # [n, 3, 3] initial body rotation (also Rwb0)
    twb: np.ndarray           # [n, 3]
    Rcw: np.ndarray           # [n, 3, 3] raw camera pose
    tcw: np.ndarray           # [n, 3]
    Rcb: np.ndarray           # [n, 3, 3]
    tcb: np.ndarray           # [n, 3]
    fixed: np.ndarray         # [n] bool
    edge_ij: np.ndarray       # [E, 2] int32: vertex 0 (i), vertex 1 (j)
    dR: np.ndarray            # [E, 3, 3]
    dt: np.ndarray            # [E, 3]
    info_diag: tuple = INFO_4DOF

    def as_struct(self, iterations=20, lambda_init=0.0, solve_mode=capi.OSH_PGO_SOLVE_ENVELOPE):
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        self._keep = (f64(self.Rwb), f64(self.twb), f64(self.Rcw), f64(self.tcw), f64(self.Rcb), f64(self.tcb),
                      np.ascontiguousarray(self.fixed, dtype=np.uint8), np.ascontiguousarray(self.edge_ij, dtype=np.int32).reshape(-1),
                      f64(self.dR), f64(self.dt))
        Rwb, twb, Rcw, tcw, Rcb, tcb, fx, eij, dR, dt = self._keep
        P = capi.ptr
        return capi.Pgo4Problem(len(fx), P(Rwb, capi.c_double_p), P(twb, capi.c_double_p), P(Rcw, capi.c_double_p), P(tcw, capi.c_double_p),
                                P(Rcb, capi.c_double_p), P(tcb, capi.c_double_p), P(fx, capi.c_uint8_p), len(eij) // 2,
                                P(eij, capi.c_int32_p), P(dR, capi.c_double_p), P(dt, capi.c_double_p),
                                (C.c_double * 6)(*[float(x) for x in self.info_diag]), iterations, lambda_init, solve_mode)


@dataclass
class Pgo4ResultArrays:
    Rcw: np.ndarray           # [n, 3, 3]
    tcw: np.ndarray           # [n, 3]
    Rwb: np.ndarray           # [n, 3, 3]
    twb: np.ndarray           # [n, 3]
    iterations: int
    trials: int
    chi2_initial: float
    chi2_final: float
    lambda_init_used: float
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

    def solve4(self, g: Pgo4Graph, iterations=20, lambda_init=0.0, dense=False) -> Pgo4ResultArrays:
        """optimize(iterations) of a 4-DoF graph; lambda_init = 0 is g2o's computeLambdaInit."""
        prob = g.as_struct(iterations, lambda_init, capi.OSH_PGO_SOLVE_DENSE if dense else capi.OSH_PGO_SOLVE_ENVELOPE)
        n = len(g.fixed)
        Rcw, tcw, Rwb, twb = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3))
        res = capi.Pgo4Result()
        res.Rcw, res.tcw = capi.ptr(Rcw, capi.c_double_p), capi.ptr(tcw, capi.c_double_p)
        res.Rwb, res.twb = capi.ptr(Rwb, capi.c_double_p), capi.ptr(twb, capi.c_double_p)
        capi.check(self.lib.osh_pgo4_solve(self.ctx, C.byref(prob), C.byref(res)), "osh_pgo4_solve", self.lib)
        return Pgo4ResultArrays(Rcw, tcw, Rwb, twb, res.iterations, res.trials, res.chi2_initial, res.chi2_final, res.lambda_init_used,
                                res.envelope_entries, res.envelope_tiles, res.tall_columns)


    def linearize4(self, g: Pgo4Graph):
        """chi2, H (dense, both triangles) and b = -J^T Omega e of the first linearisation of a 4-DoF graph."""
        prob = g.as_struct()
        N = 4 * int(np.count_nonzero(~np.asarray(g.fixed, dtype=bool)))
        H = np.zeros((N, N))
        b = np.zeros(max(N, 1))
        chi2 = np.zeros(1)
        capi.check(self.lib.osh_pgo4_linearize(self.ctx, C.byref(prob), capi.ptr(H, capi.c_double_p), capi.ptr(b, capi.c_double_p),
                                               capi.ptr(chi2, capi.c_double_p)), "osh_pgo4_linearize", self.lib)
        return float(chi2[0]), H, b[:N]
