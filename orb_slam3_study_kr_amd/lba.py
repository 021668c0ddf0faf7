"""Python driver over the local-BA C-ABI (include/orbslam3_hip.h, osh_lba_*).

Thin plumbing only: every number is computed by the HIP kernels that csrc/lba_device.hip launches
(csrc/lba_lm_kernels.h, lba_schur_items.h, lba_reduce_solve.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .synth import LbaResultArrays, LbaWindow


class LbaSolver:
    """Owns one ``osh_lba_ctx`` (one HIP device + stream)."""

    def __init__(self, device: int = 0):
        self.lib = capi.load_library()
        self.ctx = C.c_void_p()
        capi.check(self.lib.osh_lba_create(device, C.byref(self.ctx)), "osh_lba_create", self.lib)
        self._windows: list[LbaWindow] = []
        self._problems = None

    def close(self):
        if self.ctx:
            self.lib.osh_lba_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- batch life cycle -------------------------------------------------------------------
    def upload(self, windows: list[LbaWindow]):
        self._windows = list(windows)
        arr = (capi.LbaProblem * len(windows))()
        for i, w in enumerate(windows):
            arr[i] = w.as_struct()
        self._problems = arr
        capi.check(self.lib.osh_lba_upload(self.ctx, len(windows), arr), "osh_lba_upload", self.lib)

    def optimize(self):
        capi.check(self.lib.osh_lba_optimize(self.ctx), "osh_lba_optimize", self.lib)

    def set_pack_mode(self, mode: int):
        """0: uploads are packed by HIP kernels (default), 1: by host threads (csrc/lba_pack.h), -1: default rules."""
        capi.check(self.lib.osh_lba_set_pack_mode(self.ctx, mode), "osh_lba_set_pack_mode", self.lib)

    def pack_compare(self, windows) -> dict:
        """Packs ``windows`` with the device packer and the host packer and compares the two layouts byte by byte."""
        arr = (capi.LbaProblem * len(windows))()
        for i, w in enumerate(windows):
            arr[i] = w.as_struct()
        st = np.zeros(4, dtype=np.int64)
        capi.check(self.lib.osh_lba_pack_compare(self.ctx, len(windows), arr, capi.ptr(st, capi.c_int64_p)), "osh_lba_pack_compare", self.lib)
        return dict(bytes=int(st[0]), sections=int(st[1]), items=int(st[2]), records=int(st[3]))

    # -- the same life cycle on prepared ctypes arrays (bench.py's end-to-end pipeline: nothing but the C-ABI calls is timed) --
    def prepare(self, windows: list[LbaWindow]):
        """(problem array, result array, result holders) for upload_prepared / download_prepared."""
        n = len(windows)
        probs = (capi.LbaProblem * n)()
        for i, w in enumerate(windows):
            probs[i] = w.as_struct()
        outs = [LbaResultArrays(w) for w in windows]
        res = (capi.LbaResult * n)()
        for i, o in enumerate(outs):
            o.bind(res[i])
        return probs, res, outs

    def upload_prepared(self, windows, probs):
        self._windows = windows
        self._problems = probs
        capi.check(self.lib.osh_lba_upload(self.ctx, len(windows), probs), "osh_lba_upload", self.lib)

    def download_prepared(self, res):
        capi.check(self.lib.osh_lba_download(self.ctx, len(res), res), "osh_lba_download", self.lib)

    def upload_times(self) -> dict:
        ms = np.zeros(2, dtype=np.float64)
        capi.check(self.lib.osh_lba_get_upload_times(self.ctx, capi.ptr(ms, capi.c_double_p)), "osh_lba_get_upload_times", self.lib)
        return dict(pack_ms=float(ms[0]), copy_ms=float(ms[1]))

    def pack_profile(self) -> dict:
        ms = np.zeros(30, dtype=np.float64)
        capi.check(self.lib.osh_lba_get_pack_profile(self.ctx, capi.ptr(ms, capi.c_double_p)), "osh_lba_get_pack_profile", self.lib)
        names = ("histogram", "offsets", "scatter", "order", "units", "", "", "", "unit_keys", "grouping", "compaction", "key_sort", "ranks", "greedy_merge",
                 "place_units", "renumber", "chunks", "slot_bytes", "arena0", "contrib_counts", "items_records", "contrib_slots", "", "")
        return dict(h2d_ms=float(ms[0]), pre1_ms=float(ms[1]), pre2_ms=float(ms[2]), post_ms=float(ms[3]), staged_bytes=int(ms[4]), on_device=bool(ms[5]),
                    kcycles={n: round(float(c) / 1e3, 1) for n, c in zip(names, ms[6:]) if n})

    def download(self) -> list[LbaResultArrays]:
        n = len(self._windows)
        outs = [LbaResultArrays(w) for w in self._windows]
        arr = (capi.LbaResult * n)()
        for i, o in enumerate(outs):
            o.bind(arr[i])
        capi.check(self.lib.osh_lba_download(self.ctx, n, arr), "osh_lba_download", self.lib)
        return [o.read_scalars(arr[i]) for i, o in enumerate(outs)]

    def solve(self, windows: list[LbaWindow]) -> list[LbaResultArrays]:
        self.upload(windows)
        self.optimize()
        return self.download()

    # -- local inertial BA (one persistent block per window, csrc/liba_device.hip) ---------------
    def solve_inertial(self, windows):
        from .synth_inertial import LibaResultArrays
        n = len(windows)
        probs = (capi.LibaProblem * n)()
        for i, w in enumerate(windows):
            probs[i] = w.as_struct()
        outs = [LibaResultArrays(w) for w in windows]
        arr = (capi.LibaResult * n)()
        for i, o in enumerate(outs):
            o.bind(arr[i])
        capi.check(self.lib.osh_liba_solve(self.ctx, n, probs, arr), "osh_liba_solve", self.lib)
        return [o.read_scalars(arr[i]) for i, o in enumerate(outs)]

    def inertial_profile(self):
        """(blocks per window, shader-clock cycles per phase of window 0) of the last solve_inertial on this thread."""
        grp = C.c_int32(0)
        cyc = np.zeros(8, dtype=np.int64)
        capi.check(self.lib.osh_liba_get_profile(C.byref(grp), capi.ptr(cyc, capi.c_int64_p)), "osh_liba_get_profile", self.lib)
        names = ("linearise", "assembly", "dinv", "schur", "ldlt", "backsub", "errors", "outputs")
        return int(grp.value), dict(zip(names, (int(c) for c in cyc)))

    # -- parity / debug aids ------------------------------------------------------------------
    def linearize(self, window: int = 0) -> dict:
        w = self._windows[window]
        P, L, E = w.n_free, w.n_points, w.n_edges
        out = dict(Hpp=np.zeros((P, 6, 6)), bp=np.zeros((P, 6)), Hll=np.zeros((L, 3, 3)), bl=np.zeros((L, 3)),
                   Hpl=np.zeros((E, 6, 3)), chi2=np.zeros(E))
        rc = C.c_double(0)
        d = capi.c_double_p
        capi.check(self.lib.osh_lba_linearize(self.ctx, window, capi.ptr(out["Hpp"], d), capi.ptr(out["bp"], d),
                                              capi.ptr(out["Hll"], d), capi.ptr(out["bl"], d), capi.ptr(out["Hpl"], d),
                                              capi.ptr(out["chi2"], d), C.cast(C.byref(rc), d)),
                   "osh_lba_linearize", self.lib)
        out["robust_chi2"] = rc.value
        return out

    def debug_trial(self, window: int, lam: float):
        w = self._windows[window]
        n = 6 * w.n_free
        S, bs, x = np.zeros((n, n)), np.zeros(n), np.zeros(n + 3 * w.n_points)
        d = capi.c_double_p
        capi.check(self.lib.osh_lba_debug_trial(self.ctx, window, lam, capi.ptr(S, d), capi.ptr(bs, d), capi.ptr(x, d)),
                   "osh_lba_debug_trial", self.lib)
        return S, bs, x

    def linearize_inertial(self, w) -> dict:
        """``osh_liba_linearize``: the system of the first buildSystem of one inertial window in the layout of the oracle's
        liba_linearize, and the path taken (NB, G, C, il, n_colours)."""
        n, L, E = 15 * w.n_opt, w.n_points, w.n_edges
        out = dict(H=np.zeros((n, n)), b=np.zeros(n + 3 * L), Hll=np.zeros((L, 3, 3)), Hpl=np.zeros((E, 6, 3)))
        chi, info = np.zeros(1), np.zeros(5, dtype=np.int32)
        p, d = w.as_struct(), capi.c_double_p
        capi.check(self.lib.osh_liba_linearize(self.ctx, C.byref(p), capi.ptr(out["H"], d), capi.ptr(out["b"], d), capi.ptr(out["Hll"], d),
                                               capi.ptr(out["Hpl"], d), capi.ptr(chi, d), capi.ptr(info, capi.c_int32_p)),
                   "osh_liba_linearize", self.lib)
        out["chi2"] = float(chi[0])
        out["info"] = dict(zip(("NB", "G", "C", "il", "n_colours"), (int(k) for k in info)))
        return out

    def inertial_edges(self, w):
        """``osh_liba_inertial_edges``: (J [links][9][24], -rho' W r [links][9], rho' [links]) of the first linearisation."""
        NL = w.n_links
        J, Wr, rho1 = np.zeros((NL, 9, 24)), np.zeros((NL, 9)), np.zeros(NL)
        p, d = w.as_struct(), capi.c_double_p
        capi.check(self.lib.osh_liba_inertial_edges(self.ctx, C.byref(p), capi.ptr(J, d), capi.ptr(Wr, d), capi.ptr(rho1, d)),
                   "osh_liba_inertial_edges", self.lib)
        return J, Wr, rho1

    def debug_trial_inertial(self, w, lam: float = 0.0):
        """``osh_liba_debug_trial``: (S, bs, keyframe step, landmark step, lambda used) of the first trial; lam <= 0: the default lambda."""
        n, L = 15 * w.n_opt, w.n_points
        S, bs, x, xl, used = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros((L, 3)), np.zeros(1)
        p, d = w.as_struct(), capi.c_double_p
        capi.check(self.lib.osh_liba_debug_trial(self.ctx, C.byref(p), float(lam), capi.ptr(S, d), capi.ptr(bs, d), capi.ptr(x, d), capi.ptr(xl, d),
                                                 capi.ptr(used, d)), "osh_liba_debug_trial", self.lib)
        return S, bs, x, xl, float(used[0])

    # -- profiling ------------------------------------------------------------------------------
    def optimize_poses(self, frames):
        """``osh_pose_optimize``: Optimizer::PoseOptimization's four rounds for every frame of the batch, one block per frame."""
        from .synth import PoseResultArrays
        n = len(frames)
        probs = (capi.PoseProblem * n)(*[f.as_struct() for f in frames])
        res = [PoseResultArrays(f) for f in frames]
        rs = (capi.PoseResult * n)()
        for r, a in zip(rs, res):
            a.bind(r)
        capi.check(self.lib.osh_pose_optimize(self.ctx, n, probs, rs), "osh_pose_optimize", self.lib)
        return [a.read_scalars(r) for r, a in zip(rs, res)]

    def optimize_sim3(self, problems):
        """``osh_sim3_optimize``: Optimizer::OptimizeSim3's two rounds for every problem of the batch, one block per problem.

        `problems` are packs of ``synth_sim3`` (dicts with X1c, X2c, obs1, obs2, info1, info2, cameras, S12, th2, fix_scale)."""
        from .synth_sim3 import bind_result, problem, read_result
        n = len(problems)
        keep = []
        probs = (capi.Sim3Problem * n)(*[problem(p, keep) for p in problems])
        rs = (capi.Sim3Result * n)()
        arrs = []
        for k, p in enumerate(problems):
            r, a = bind_result(len(p["index"]))
            rs[k] = r
            arrs.append(a)
        capi.check(self.lib.osh_sim3_optimize(self.ctx, n, probs, rs), "osh_sim3_optimize", self.lib)
        return [read_result(rs[k], arrs[k]) for k in range(n)]

    def linearize_sim3(self, pk):
        """``osh_sim3_linearize``: robust chi2, H (7x7) and b of the first linearisation of one problem."""
        H = np.zeros((7, 7)); b = np.zeros(7); chi2 = C.c_double(0.0)
        from .synth_sim3 import problem
        keep = []
        p = problem(pk, keep)
        capi.check(self.lib.osh_sim3_linearize(self.ctx, C.byref(p), capi.ptr(H, capi.c_double_p), capi.ptr(b, capi.c_double_p),
                                               C.byref(chi2)), "osh_sim3_linearize", self.lib)
        return chi2.value, H, b

    def optimize_poses_inertial(self, frames):
        """``osh_posei_optimize``: Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame for every frame of the batch."""
        from .synth_inertial import PoseiResultArrays
        n = len(frames)
        probs = (capi.PoseiProblem * n)(*[f.as_struct() for f in frames])
        res = [PoseiResultArrays(f) for f in frames]
        rs = (capi.PoseiResult * n)()
        for r, a in zip(rs, res):
            a.bind(r)
        capi.check(self.lib.osh_posei_optimize(self.ctx, n, probs, rs), "osh_posei_optimize", self.lib)
        return [a.read(r, f.mode) for r, a, f in zip(rs, res, frames)]

    def linearize_pose_inertial(self, frame):
        """``osh_posei_linearize``: H and b of the first Gauss-Newton iteration of one frame ([current P V G A | previous P V G A])."""
        n = 30 if frame.mode == 1 else 15
        H, b = np.zeros((n, n)), np.zeros(n)
        p = frame.as_struct()
        capi.check(self.lib.osh_posei_linearize(self.ctx, C.byref(p), capi.ptr(H, capi.c_double_p), capi.ptr(b, capi.c_double_p)),
                   "osh_posei_linearize", self.lib)
        return H, b

    def plan_stats(self) -> dict:
        st = np.zeros(8, dtype=np.int64)
        capi.check(self.lib.osh_lba_get_plan_stats(self.ctx, capi.ptr(st, capi.c_int64_p)), "osh_lba_get_plan_stats", self.lib)
        return dict(items=int(st[0]), sym_items=int(st[1]), mfma_per_pass=int(st[2]), useful_blocks=int(st[3]), contributions=int(st[4]),
                    reduce_entries=int(st[5]), records=int(st[6]), rhs_contributions=int(st[7]))

    def get_solver(self) -> dict:
        """Which factorisation the reduced systems of the last upload take: big (csrc/big_solve.h) or k_solve<nb, threads>."""
        out = np.zeros(4, dtype=np.int32)
        capi.check(self.lib.osh_lba_get_solver(self.ctx, capi.ptr(out, capi.c_int32_p)), "osh_lba_get_solver", self.lib)
        return dict(big=bool(out[0]), nb=int(out[1]), threads=int(out[2]), lds_bytes=int(out[3]))

    def set_profiling(self, enable: bool):
        capi.check(self.lib.osh_lba_set_profiling(self.ctx, int(enable)), "osh_lba_set_profiling", self.lib)

    def profile(self) -> dict:
        """{short kernel name: (launches, total ms)} measured with HIP events on the solver's stream."""
        launches = np.zeros(capi.OSH_K_COUNT, dtype=np.int64)
        ms = np.zeros(capi.OSH_K_COUNT, dtype=np.float64)
        capi.check(self.lib.osh_lba_get_profile(self.ctx, capi.ptr(launches, capi.c_int64_p), capi.ptr(ms, capi.c_double_p)),
                   "osh_lba_get_profile", self.lib)
        return {capi.KERNEL_NAMES[k]: (int(launches[k]), float(ms[k])) for k in range(capi.OSH_K_COUNT)}


ITEM_MAX_LM = 256   # csrc/schur_plan.h:kItemMaxLm


def pack_cuts(n_windows: int, use_env: bool = False) -> tuple[int, int]:
    """(landmarks per Schur item, edges per landmark chunk) of a call of n_windows windows: its size class, or with use_env what an
    upload would use under OSH_LBA_ITEM_MAX / OSH_LBA_CHUNK_EDGES."""
    lib = capi.load_library()
    out = np.zeros(2, dtype=np.int32)
    capi.check(lib.osh_lba_pack_cuts(int(n_windows), int(use_env), capi.ptr(out, capi.c_int32_p)), "osh_lba_pack_cuts", lib)
    return int(out[0]), int(out[1])


def schur_plan_check(window: LbaWindow, item_max: int = 0) -> dict:
    """Host-only check of the Schur plan of one window cut at item_max landmarks per item (0: a one-window call's): raises on a
    plan that does not cover every observer pair exactly once, returns its statistics."""
    lib = capi.load_library()
    pr = window.as_struct()
    st = np.zeros(8, dtype=np.int64)
    capi.check(lib.osh_lba_schur_plan_stats_cut(C.byref(pr), int(item_max), capi.ptr(st, capi.c_int64_p)), "osh_lba_schur_plan_stats_cut", lib)
    return dict(items=int(st[0]), sym_items=int(st[1]), records=int(st[2]), contributions=int(st[3]), rhs_contributions=int(st[4]),
                mfma_per_pass=int(st[5]), useful_blocks=int(st[6]), reduce_entries=int(st[7]))


def pack_check(windows, item_max: int = 0, chunk_edges: int = 0, threads: int = 0) -> dict:
    """Host-only check of the batch packer on `windows`, cut as given (0: as an upload of that many windows)."""
    lib = capi.load_library()
    arr = (capi.LbaProblem * len(windows))(*[w.as_struct() for w in windows])
    st = np.zeros(8, dtype=np.int64)
    capi.check(lib.osh_lba_pack_check_cut(len(windows), arr, int(threads), int(item_max), int(chunk_edges), capi.ptr(st, capi.c_int64_p), None),
               "osh_lba_pack_check_cut", lib)
    return dict(items=int(st[0]), sym_items=int(st[1]), records=int(st[2]), contributions=int(st[3]), chunks=int(st[4]),
                staging_bytes=int(st[5]), merged_pairs=int(st[6]), reduce_entries=int(st[7]))


def schur_plan_shapes(window: LbaWindow, item_max: int = 0) -> tuple[dict, int, int]:
    """Item shapes of the Schur plan of one window, on the CPU: ({(sym, nx, ny, landmarks): items}, matrix-pipe cycles of one pass
    with whole tiles, the same with the symmetric items' four-block instructions).  item_max 0: what a call with one window uses."""
    lib = capi.load_library()
    pr = window.as_struct()
    hist = np.zeros((2, 9, 9, ITEM_MAX_LM + 1), dtype=np.int64)
    cyc = np.zeros(2, dtype=np.int64)
    capi.check(lib.osh_lba_schur_plan_shapes(C.byref(pr), int(item_max), capi.ptr(hist, capi.c_int64_p), capi.ptr(cyc, capi.c_int64_p)),
               "osh_lba_schur_plan_shapes", lib)
    return {tuple(int(v) for v in k): int(hist[tuple(k)]) for k in np.argwhere(hist)}, int(cyc[0]), int(cyc[1])


def schur_block_list(sym: bool, nx: int, ny: int, use_blocks: bool = True) -> list[tuple]:
    """Matrix instructions of one k step of an item: ("tile", ti, tj) or ("blocks", [(block row, block column, use)] * 4)
    (include/orbslam3_hip.h:osh_lba_schur_block_list)."""
    lib = capi.load_library()
    out = np.zeros((24, 16), dtype=np.int32)
    n = np.zeros(1, dtype=np.int32)
    capi.check(lib.osh_lba_schur_block_list(int(sym), nx, ny, int(use_blocks), capi.ptr(out, capi.c_int32_p), capi.ptr(n, capi.c_int32_p)),
               "osh_lba_schur_block_list", lib)
    return [("tile", int(r[1]), int(r[2])) if r[0] == 0 else ("blocks", [tuple(int(v) for v in r[4 + 3 * q:7 + 3 * q]) for q in range(4)])
            for r in out[:int(n[0])]]


def kernel_symbol(short_name: str) -> str:
    """Device kernel name (as rocprofv3 prints it) behind a short name of ``capi.KERNEL_NAMES``."""
    lib = capi.load_library()
    return lib.osh_lba_kernel_name(capi.KERNEL_NAMES.index(short_name)).decode()
