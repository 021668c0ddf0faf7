#!/usr/bin/env python3
"""Sim3 RANSAC timing: osh_orb_sim3_ransac on four shapes -- one problem of 100 correspondences x 300 iterations, one of 300 x 300
(one loop candidate at Sim3Solver's iteration cap), three such problems in one call (the candidates of one
LoopClosing::DetectCommonRegionsFromBoW), a batch of 64 -- against osh_host_sim3r_cpu, the same statements (csrc/sim3_ransac.h)
compiled for the host at the library's optimisation level and run on one thread of the same machine.  That is not the reference's
Eigen build: the project builds without Eigen and has no build of the reference to time.  The problems carry 30 % outliers; every
call forms and scores all its hypotheses whatever the scene (the entry has no early exit).  The device call is split into staging,
upload, kernels and download by its own phase clocks (osh_orb_sim3_ransac_get_times under osh_orb_set_profiling, which synchronises
between the phases) and also timed unprofiled; every timed call ends in the call's own stream synchronisation.  --warmup calls first,
then --reps timed calls, median and spread (max - min) in ms.  --json writes the rows."""
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
from orb_slam3_study_kr_amd import synth_sim3_ransac as ss  # noqa: E402


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
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<66} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    def scene(k, n=300):
        return ss.make_problem(seed=100 + k, n=n, iterations=300, camera_type1=ss.KB8 if k % 2 else ss.PINHOLE,
                               camera_type2=ss.KB8 if k % 2 else ss.PINHOLE, fix_scale=k % 3 == 0, min_inliers=20)

    shapes = [("1 x (100 x 300)", [scene(0, 100)]), ("1 x (300 x 300)", [scene(0)]), ("3 x (300 x 300)", [scene(k) for k in range(3)]),
              ("64 x (300 x 300)", [scene(k) for k in range(64)])]
    with orb.OrbMatcher(0) as m:
        for label, pbs in shapes:
            cp, cr, _keep, outs = orb.sim3_ransac_args(pbs)

            def gpu():
                capi.check(lib.osh_orb_sim3_ransac(m.ctx, len(pbs), cp, cr), "osh_orb_sim3_ransac", lib)
            ms, sp = timed(gpu, a.reps, a.warmup)
            row(f"{label}: device call", ms, sp, problems=len(pbs), problems_per_s=len(pbs) * 1e3 / ms)
            m.set_profiling(True)
            phases = []
            for k in range(a.warmup + a.reps):
                gpu()
                if k >= a.warmup:
                    phases.append(m.sim3_ransac_times())
            m.set_profiling(False)
            phases = np.array(phases)
            for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                row(f"{label}:   {phase}", float(np.median(phases[:, k])), float(phases[:, k].max() - phases[:, k].min()))
            hp, hr, _hkeep, houts = orb.sim3_ransac_args(pbs)
            inner = C.c_double(0)

            def cpu():
                if host.osh_host_sim3r_cpu(len(pbs), hp, hr, C.byref(inner)) != 0:
                    raise RuntimeError("osh_host_sim3r_cpu")
            cms, csp = timed(cpu, a.cpu_reps, 1)
            row(f"{label}: CPU, one thread, the same statements", cms, csp, problems=len(pbs), problems_per_s=len(pbs) * 1e3 / cms)
            same = all(np.array_equal(o[k], h[k]) for o, h in zip(outs, houts) for k in ("first_hit", "n_records", "record", "record_count", "record_mask"))
            hits = sum(int(o["first_hit"][0]) >= 0 for o in outs)
            print(f"  ({hits} hits of {len(pbs)}; device equals CPU in records, counts and masks: {same}; device / CPU = {ms / cms:.4f})")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
