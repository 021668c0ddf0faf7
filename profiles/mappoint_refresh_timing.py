#!/usr/bin/env python3
"""Map point refresh timing: osh_orb_refresh_map_points (MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth) on
(a) one keyframe's 1000 points from the generator's distribution, (b) 30 such batches in one call -- against
osh_host_mappoint_refresh_cpu, the same statements (csrc/mappoint_refresh.h) compiled for the host at the library's optimisation
level and run on one thread of the same machine.  That CPU run is the baseline.  The device call is timed by wall clock
unprofiled (every call ends in its own stream synchronisation) and split into staging, upload, kernels and download by its phase
clock (osh_orb_set_profiling on, which synchronises between the phases).  --warmup calls first, then --reps timed calls, median
and spread (max - min) in ms.  The argument and result arrays are built once, as a caller that keeps its buffers does.  Both
sides are checked against each other bit for bit before anything is timed.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/mappoint_refresh_timing.py --reps 50"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import mappoint_numpy as mn  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_mappoints as sm  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--batches", default="1,30")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    if lib.osh_device_count() < 1:
        raise SystemExit("mappoint_refresh_timing: no HIP device visible")
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<62} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    n_max = max(int(b) for b in a.batches.split(","))
    distinct = [sm.make_batch(700 + k, a.points) for k in range(n_max)]
    with orb.OrbMatcher(0) as m:
        for n_b in (int(b) for b in a.batches.split(",")):
            batches = distinct[:n_b]
            points, entries = sum(b.n_points for b in batches), sum(b.n_entries for b in batches)
            over = sum(int((b.counts() > 64).sum()) for b in batches)
            name = f"{n_b} x {a.points} points"
            cb, cr, _keep, outs = orb.mappoint_args(batches)
            hb, hr, _hkeep, houts = orb.mappoint_args(batches)

            def device():
                capi.check(lib.osh_orb_refresh_map_points(m.ctx, n_b, cb, cr), "osh_orb_refresh_map_points", lib)
            inner = C.c_double(0)
            loops = []

            def cpu():
                if host.osh_host_mappoint_refresh_cpu(n_b, hb, hr, C.byref(inner)) != 0:
                    raise RuntimeError("osh_host_mappoint_refresh_cpu")
                loops.append(inner.value)
            device(); cpu()
            for got, exp in zip(outs, houts):
                assert mn.same_bits(got, exp) == [], name
            ms, sp = timed(device, a.reps, a.warmup)
            row(f"{name}: osh_orb_refresh_map_points (wall)", ms, sp, points=points, entries=entries, block_class_points=over, points_per_s=points * 1e3 / ms)
            m.set_profiling(True)
            phases = []
            for k in range(a.warmup + a.reps):
                device()
                if k >= a.warmup:
                    phases.append(m.refresh_map_points_times())
            m.set_profiling(False)
            ph = np.array(phases)
            for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                row(f"{name}:   {phase}", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
            total = float(np.median(ph.sum(axis=1)))
            row(f"{name}:   sum of the phases (profiled call)", total, float(ph.sum(axis=1).max() - ph.sum(axis=1).min()),
                kernel_share=float(np.median(ph[:, 2])) / total)
            loops.clear()
            cms, csp = timed(cpu, a.cpu_reps, 2)
            inner_ms = np.array(loops[2:])
            row(f"{name}: CPU, one thread (wall)", cms, csp, points_per_s=points * 1e3 / cms)
            row(f"{name}: CPU, one thread, the loops over the points", float(np.median(inner_ms)), float(inner_ms.max() - inner_ms.min()))
            print(f"  ({points} points, {entries} entries, {over} points above a wavefront; device / CPU = {ms / cms:.3f}; "
                  f"kernels are {100 * float(np.median(ph[:, 2])) / total:.0f} % of the profiled call)")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
