#!/usr/bin/env python3
"""ORBextractor::operator() timing after the detector: osh_orb_describe (the 7x7 blur of the levels and the steered-BRIEF
descriptors) by token on 752 x 480 pyramids of 8 levels with the keypoints ComputeKeyPointsOctTree of the stand-in class returns at
nfeatures = 1500 -- one frame per call, the stereo pair, a batch of 64 -- and operator() end to end through the stand-in class,
against osh_host_orb_describe_cpu: the same statements (csrc/orb_brief.h) compiled for the host at the library's optimisation level
and run on one thread of the same machine.  That CPU run is the same header, not OpenCV's GaussianBlur and computeDescriptors, which
cannot be built here.  The device calls are split into staging, upload, kernels and download by their own phase clocks
(osh_orb_set_profiling on, which synchronises between the phases) and also timed unprofiled; every timed call ends in the call's
own stream synchronisation.  --warmup calls first, then --reps timed calls, median and spread (max - min) in ms.  --json writes
the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/brief_timing.py --reps 50"""
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

import brief_numpy as bn  # noqa: E402
from orb_slam3_study_kr_amd import capi, host, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_fast as sf  # noqa: E402


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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--batches", default="1,2,64")
    ap.add_argument("--nfeatures", type=int, default=1500)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, hostlib = capi.load_library(), capi.load_host_library()
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<62} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    pattern = orb.standin_pattern()
    distinct = []
    for k in range(4):
        frame = sf.make_frame(900 + k, 752, 480, 8)
        r = host.orbextractor_compute_keypoints(frame.pyramid, nfeatures=a.nfeatures, border=19)
        level = np.repeat(np.arange(8), r["level_count"]).astype(np.int32)
        distinct.append((frame, dict(xy=r["xy"], level=level, angle=r["angle"], pattern=pattern)))
    exp0 = bn.describe(distinct[0][0].pyramid, distinct[0][1]["xy"], distinct[0][1]["level"], distinct[0][1]["angle"], pattern)
    with orb.OrbMatcher(0) as m:
        for batch in (int(b) for b in a.batches.split(",")):
            frames = [distinct[k % len(distinct)] for k in range(batch)]
            name = f"{batch} x 752x480x8"
            n_keys = sum(len(f[1]["level"]) for f in frames)
            sized = m.fast_detect([f[0] for f in frames])
            items = [dict(f[1], token=sized[j]["token"]) for j, f in enumerate(frames)]
            cf, cr, _keep, outs = orb.describe_args(items)

            def describe():
                capi.check(lib.osh_orb_describe(m.ctx, batch, cf, cr), "osh_orb_describe", lib)
            ms, sp = timed(describe, a.reps, a.warmup)
            row(f"{name}: osh_orb_describe by token", ms, sp, keypoints=n_keys, frames_per_s=batch * 1e3 / ms)
            bn.assert_same(outs[0], exp0, name, debug=False)
            pf, pr, _pkeep, pouts = orb.describe_args([dict(f[1], pyramid=f[0].pyramid) for f in frames])
            ms_p, sp = timed(lambda: capi.check(lib.osh_orb_describe(m.ctx, batch, pf, pr), "osh_orb_describe", lib), a.reps, a.warmup)
            row(f"{name}: osh_orb_describe with its pyramid", ms_p, sp, upload_bytes=sum(p.size for f in frames for p in f[0].pyramid))
            bn.assert_same(pouts[0], exp0, name + " (pyramid)", debug=False)
            m.set_profiling(True)
            phases = []
            for k in range(a.warmup + a.reps):
                describe()
                if k >= a.warmup:
                    phases.append(m.describe_times())
            m.set_profiling(False)
            ph = np.array(phases)
            for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                row(f"{name}:   describe {phase}", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
            if batch > 2:
                continue     # the CPU rows scale with the number of frames
            inner = C.c_double(0)
            loops = []

            def cpu():
                if hostlib.osh_host_orb_describe_cpu(batch, pf, pr, C.byref(inner)) != 0:
                    raise RuntimeError("osh_host_orb_describe_cpu")
                loops.append(inner.value)
            cms, csp = timed(cpu, a.cpu_reps, 1)
            row(f"{name}: CPU, one thread, blur + descriptors (same header)", cms, csp, frames_per_s=batch * 1e3 / cms)
            bn.assert_same(pouts[0], exp0, name + " (CPU)", debug=False)
            print(f"  ({n_keys} keypoints; device by token / CPU = {ms / cms:.4f})")
    # operator() end to end through the stand-in class: its ComputePyramid and octree doubles on the host, detect, orientation,
    # describe by token and the write-back; the call alone, timed inside the C++ wrapper
    img = sf.make_image(900, 480, 752)
    ts = [orb.extract(img, nfeatures=a.nfeatures, nlevels=8)["call_ms"] for _ in range(a.warmup + max(a.reps // 5, 3))][a.warmup:]
    row("operator() of the stand-in class, 752x480, 8 levels", float(np.median(ts)), float(max(ts) - min(ts)))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
