#!/usr/bin/env python3
"""Frame::ComputeStereoMatches timing: osh_orb_stereo_match on one 752x480 frame with ~1500 + 1500 keypoints (8 levels), split into
staging (pyramid rows into pinned memory), upload, kernels and download by the call's own phase clocks (osh_orb_set_profiling on,
which synchronises between the phases), the same call unprofiled, batches of 8 / 64 / 256 frames as frames/s, and the single-thread
C++ restatement of the test library on the same host.  Every timed call ends in the call's own stream synchronisation; --warmup calls
first, then --reps timed calls, median and spread (max - min) in ms.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/stereo_timing.py --batches "" --reps 50"""
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

import stereo_numpy as sn  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_stereo as ss  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--border", type=int, default=19, help="pixels around every level (the reference's EDGE_THRESHOLD): strided rows")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    rows = []
    distinct = [ss.make_stereo_frame(500 + k, n_left=1500) for k in range(8)]
    fr = distinct[0]
    print(f"frame: {fr.left_xy.shape[0]} left, {fr.right_xy.shape[0]} right keypoints, {fr.n_levels} levels, "
          f"{sum(m.size for m in fr.left_pyramid) / 1e6:.2f} MB of pixels per side")
    with orb.OrbMatcher(0) as m:
        cf, cr, keep, outs = orb.stereo_args([fr], False, [a.border])

        def one():
            capi.check(lib.osh_orb_stereo_match(m.ctx, 1, cf, cr), "osh_orb_stereo_match", lib)
        med, spread = timed(one, a.reps, a.warmup)
        exp = sn.compute_stereo_matches(fr)
        sn.assert_same(outs[0], exp, keys=("u_right", "depth"), what="timed frame")
        rows.append(dict(what="single frame call", ms=med, spread_ms=spread))
        print(f"single frame, one call                 {med:8.3f} ms  +- {spread:.3f}")
        m.set_profiling(True)
        phases = []
        for k in range(a.warmup + a.reps):
            one()
            if k >= a.warmup:
                phases.append(m.stereo_times())
        m.set_profiling(False)
        phases = np.array(phases)
        for k, name in enumerate(("staging", "upload", "kernels", "download")):
            pm, ps = float(np.median(phases[:, k])), float(phases[:, k].max() - phases[:, k].min())
            rows.append(dict(what=f"single frame {name}", ms=pm, spread_ms=ps))
            print(f"single frame, {name:<24} {pm:8.3f} ms  +- {ps:.3f}")
        h, hkeep = sn.host_input(fr)
        host = capi.load_host_library()
        u, d = np.zeros(h.n_left, np.float32), np.zeros(h.n_left, np.float32)
        ms = C.c_double(0)
        none32, none8 = C.cast(None, capi.c_int32_p), C.cast(None, capi.c_uint8_p)
        cpu = []

        def cpu_call():
            host.osh_host_stereo_restatement(C.byref(h), capi.ptr(u, capi.c_float_p), capi.ptr(d, capi.c_float_p), none32, none32, none32,
                                             none32, none8, none8, none32, C.byref(ms))
            cpu.append(ms.value)
        timed(cpu_call, a.reps, a.warmup)
        cpu = cpu[a.warmup:]
        rows.append(dict(what="single frame C++ restatement, one thread", ms=float(np.median(cpu)), spread_ms=float(max(cpu) - min(cpu))))
        print(f"single frame, C++ restatement 1 thread {np.median(cpu):8.3f} ms  +- {max(cpu) - min(cpu):.3f}")
        cpu_fps = 1e3 / float(np.median(cpu))
        for nb in [int(v) for v in a.batches.split(",") if v]:
            frames = [distinct[k % len(distinct)] for k in range(nb)]
            bf_, br_, bkeep, bouts = orb.stereo_args(frames, False, [a.border] * nb)

            def batch():
                capi.check(lib.osh_orb_stereo_match(m.ctx, nb, bf_, br_), "osh_orb_stereo_match", lib)
            reps = max(20, a.reps // max(1, nb // 8))
            bm, bs = timed(batch, reps, 3)
            rows.append(dict(what=f"batch of {nb}", ms=bm, spread_ms=bs, reps=reps, frames_per_s=nb * 1e3 / bm, cpu_frames_per_s=cpu_fps))
            print(f"batch of {nb:3d} frames ({reps} reps)          {bm:8.3f} ms  +- {bs:.3f}   {nb * 1e3 / bm:9.1f} frames/s   (one CPU thread: {cpu_fps:.1f} frames/s)", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
