#!/usr/bin/env python3
"""ORBextractor::ComputeKeyPointsOctTree timing: osh_orb_fast_detect followed by osh_orb_ic_angle (by token, for one keypoint per
distinct corner) on 752 x 480 pyramids of 8 levels -- one frame per call, the stereo pair, a batch of 64 -- against
osh_host_orb_fast_cpu / osh_host_orb_ic_angle_cpu, the same statements (csrc/orb_fast.h) compiled for the host at the library's
optimisation level and run on one thread of the same machine.  That CPU run is the baseline, not OpenCV's SIMD cv::FAST, which
cannot be built here.  The device calls are split into staging, upload, kernels and download by their own phase clocks
(osh_orb_set_profiling on, which synchronises between the phases) and also timed unprofiled; every timed call ends in the call's
own stream synchronisation.  --warmup calls first, then --reps timed calls, median and spread (max - min) in ms.  The result
arrays are sized once, as a caller that keeps its buffers does.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/fast_timing.py --reps 50"""
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

import fast_numpy as fn  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<58} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    distinct = [sf.make_frame(900 + k, 752, 480, 8) for k in range(4)]
    first, exp, (kxy, klevel), exp_angle = fn.case("vga_752x480_L8")
    distinct[0] = first
    with orb.OrbMatcher(0) as m:
        for batch in (int(b) for b in a.batches.split(",")):
            frames = [distinct[k % len(distinct)] for k in range(batch)]
            name = f"{batch} x 752x480x8"
            sized = m.fast_detect(frames)
            keys = [fn.keypoints_of(f, r) for f, r in zip(frames, sized)]
            n_out, n_keys = sum(r["n_out"] for r in sized), sum(len(k[1]) for k in keys)
            upload = sum(p.size for f in frames for p in f.pyramid)
            cf, cr, _keep, outs = orb.fast_args(frames, [(r["n_out"], r["n_cells"]) for r in sized])

            def detect():
                capi.check(lib.osh_orb_fast_detect(m.ctx, batch, cf, cr), "osh_orb_fast_detect", lib)
            detect()
            items = [dict(xy=k[0], level=k[1], token=int(cr[j].pyramid_token)) for j, k in enumerate(keys)]
            icf, icr, _ickeep, icouts = orb.ic_angle_args(items)

            def both():
                detect()
                for j in range(batch):
                    icf[j].pyramid_token = cr[j].pyramid_token
                capi.check(lib.osh_orb_ic_angle(m.ctx, batch, icf, icr), "osh_orb_ic_angle", lib)
            ms, sp = timed(detect, a.reps, a.warmup)
            row(f"{name}: osh_orb_fast_detect", ms, sp, corners=n_out, cells=sum(r["n_cells"] for r in sized), upload_bytes=upload, frames_per_s=batch * 1e3 / ms)
            ms_both, sp = timed(both, a.reps, a.warmup)
            row(f"{name}: detect + osh_orb_ic_angle by token", ms_both, sp, keypoints=n_keys, frames_per_s=batch * 1e3 / ms_both)
            fn.assert_detect_same(orb._fast_outputs(cr, outs)[0], exp, name)
            fn.assert_angles_same(icouts[0], exp_angle, name)
            m.set_profiling(True)
            phases, ic_phases = [], []
            for k in range(a.warmup + a.reps):
                both()
                if k >= a.warmup:
                    phases.append(m.fast_times())
                    ic_phases.append(m.ic_angle_times())
            m.set_profiling(False)
            for label, ph in (("detect", np.array(phases)), ("ic_angle", np.array(ic_phases))):
                for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                    row(f"{name}:   {label} {phase}", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
            if batch > 2:
                continue     # the CPU rows scale with the number of frames
            hf, hr, _hkeep, houts = orb.fast_args(frames, [(r["n_out"], r["n_cells"]) for r in sized])
            hitems = [dict(xy=k[0], level=k[1], pyramid=f.pyramid) for f, k in zip(frames, keys)]
            hicf, hicr, _hk, hicouts = orb.ic_angle_args(hitems)
            inner, inner_ic = C.c_double(0), C.c_double(0)
            loops = []

            def cpu():
                if host.osh_host_orb_fast_cpu(batch, hf, hr, C.byref(inner)) != 0 or host.osh_host_orb_ic_angle_cpu(batch, hicf, hicr, C.byref(inner_ic)) != 0:
                    raise RuntimeError("osh_host_orb_fast_cpu / osh_host_orb_ic_angle_cpu")
                loops.append((inner.value, inner_ic.value))
            cms, csp = timed(cpu, a.cpu_reps, 1)
            loops = np.array(loops[1:])
            row(f"{name}: CPU, one thread, detect + IC_Angle", cms, csp, frames_per_s=batch * 1e3 / cms)
            row(f"{name}: CPU, one thread, the detect loops", float(np.median(loops[:, 0])), float(loops[:, 0].max() - loops[:, 0].min()))
            row(f"{name}: CPU, one thread, the IC_Angle loop", float(np.median(loops[:, 1])), float(loops[:, 1].max() - loops[:, 1].min()))
            fn.assert_detect_same(orb._fast_outputs(hr, houts)[0], exp, name + " (CPU)")
            fn.assert_angles_same(hicouts[0], exp_angle, name + " (CPU)")
            print(f"  ({n_out} corners, {n_keys} keypoints, {upload} pyramid bytes; device / CPU = {ms_both / cms:.3f})")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
