#!/usr/bin/env python3
"""TwoViewReconstruction timing: osh_orb_two_view_reconstruct on three shapes -- one problem of 300 matches x 200 iterations (what
Tracking::MonocularInitialization sends per frame), one problem of 2000 matches x 200 iterations, a batch of 64 of the first --
against osh_host_two_view_cpu, the same statements (csrc/two_view.h) compiled for the host at the library's optimisation level and
run on one thread of the same machine.  That is not the reference's Eigen build: the project builds without Eigen, OpenCV and Sophus and has
no build of the reference to time.  The device call is split into staging, upload, kernels and download by its own phase clocks
(osh_orb_set_profiling on, which synchronises between the phases) and also timed unprofiled; every timed call ends in the call's own
stream synchronisation.  --warmup calls first, then --reps timed calls, median and spread (max - min) in ms.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/two_view_timing.py --reps 50"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_two_view as st  # noqa: E402


def timed(fn_, reps, warmup):
    for _ in range(warmup):
        fn_()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn_()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cpu-reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<58} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    small = st.problem(st.make_scene("general", seed=1, n=300), 200)
    shapes = [("1 x (300 x 200)", [small]), ("1 x (2000 x 200)", [st.problem(st.make_scene("general", seed=2, n=2000), 200)]),
              ("64 x (300 x 200)", [st.problem(st.make_scene("general", seed=10 + k, n=300), 200) for k in range(64)])]
    with orb.OrbMatcher(0) as m:
        for name, pbs in shapes:
            cp, cr, _keep, outs = orb.two_view_args(pbs)

            def gpu():
                capi.check(lib.osh_orb_two_view_reconstruct(m.ctx, len(pbs), cp, cr), "osh_orb_two_view_reconstruct", lib)
            ms, sp = timed(gpu, a.reps, a.warmup)
            row(f"{name}: device call", ms, sp, problems=len(pbs), problems_per_s=len(pbs) * 1e3 / ms)
            m.set_profiling(True)
            phases = []
            for k in range(a.warmup + a.reps):
                gpu()
                if k >= a.warmup:
                    phases.append(m.two_view_times())
            m.set_profiling(False)
            phases = np.array(phases)
            for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                row(f"{name}:   {phase}", float(np.median(phases[:, k])), float(phases[:, k].max() - phases[:, k].min()))
            hp, hr, _hkeep, houts = orb.two_view_args(pbs)
            inner = C.c_double(0)

            def cpu():
                if host.osh_host_two_view_cpu(len(pbs), hp, hr, C.byref(inner)) != 0:
                    raise RuntimeError("osh_host_two_view_cpu")
            cms, csp = timed(cpu, a.cpu_reps, 1)
            row(f"{name}: CPU, one thread, the same statements", cms, csp, problems=len(pbs), problems_per_s=len(pbs) * 1e3 / cms)
            same = all(np.array_equal(o[k], h[k]) for o, h in zip(outs, houts) for k in ("status", "best_h", "best_f", "n_good", "inlier"))
            accepted = sum(int(o["status"][0]) in (capi.OSH_TWOVIEW_ACCEPTED_H, capi.OSH_TWOVIEW_ACCEPTED_F) for o in outs)
            print(f"  ({accepted} accepted of {len(pbs)}; device equals CPU: {same}; device / CPU = {ms / cms:.3f})")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
