#!/usr/bin/env python3
"""LocalMapping::CreateNewMapPoints timing: osh_orb_triangulate_new_points on three shapes -- one segment of 300 matches (what the
drop-in sends per neighbour), one segment of 2000 matches, 30 segments of 300 in one call -- against
osh_host_newpoint_triangulate_cpu, the same statements (csrc/newpoint_triangulate.h) compiled for the host at the library's
optimisation level and run on one thread of the same machine.  The device call is split into staging, upload, kernel and download
by its own phase clocks (osh_orb_set_profiling on, which synchronises between the phases) and also timed unprofiled; every timed
call ends in the call's own stream synchronisation.  --warmup calls first, then --reps timed calls, median and spread (max - min)
in ms.  The segments are rectified-stereo ones (all three sources of x3D occur) unless --kind says otherwise.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/newpoints_timing.py --reps 50"""
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

import newpoints_numpy as nn  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_newpoints as sn  # noqa: E402


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
    ap.add_argument("--kind", default="stereo", choices=["mono", "stereo", "kb8", "rig"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<58} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    shapes = [("1 x 300", [sn.make_segment(700, a.kind, 300)]), ("1 x 2000", [sn.make_segment(701, a.kind, 2000)]),
              ("30 x 300", [sn.make_segment(710 + k, a.kind, 300) for k in range(30)])]
    with orb.OrbMatcher(0) as m:
        for name, segs in shapes:
            n = sum(s.n for s in segs)
            cs, cr, _keep, outs = orb.newpoint_args(segs)

            def gpu():
                capi.check(lib.osh_orb_triangulate_new_points(m.ctx, len(segs), cs, cr), "osh_orb_triangulate_new_points", lib)
            ms, sp = timed(gpu, a.reps, a.warmup)
            row(f"{name}: device call", ms, sp, matches=n, matches_per_s=n * 1e3 / ms)
            nn.assert_matches(outs[0], nn.compute(segs[0]), what=name)
            accepted = sum(int((o["stage"] == capi.OSH_NEWPOINT_ACCEPTED).sum()) for o in outs)
            m.set_profiling(True)
            phases = []
            for k in range(a.warmup + a.reps):
                gpu()
                if k >= a.warmup:
                    phases.append(m.newpoint_times())
            m.set_profiling(False)
            phases = np.array(phases)
            for k, phase in enumerate(("staging", "upload", "kernel", "download")):
                row(f"{name}:   {phase}", float(np.median(phases[:, k])), float(phases[:, k].max() - phases[:, k].min()))
            hs, hr, _hkeep, houts = orb.newpoint_args(segs)
            inner = C.c_double(0)
            loops = []

            def cpu():
                if host.osh_host_newpoint_triangulate_cpu(len(segs), hs, hr, C.byref(inner)) != 0:
                    raise RuntimeError("osh_host_newpoint_triangulate_cpu")
                loops.append(inner.value)
            cms, csp = timed(cpu, a.reps, a.warmup)
            row(f"{name}: CPU, one thread, whole call", cms, csp, matches=n, matches_per_s=n * 1e3 / cms)
            row(f"{name}: CPU, one thread, the loop over the matches", float(np.median(loops[a.warmup:])), float(max(loops[a.warmup:]) - min(loops[a.warmup:])))
            nn.assert_matches(houts[0], nn.compute(segs[0]), what=name + " (CPU)")
            print(f"  ({accepted} accepted of {n}; device / CPU = {ms / cms:.2f})")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
