#!/usr/bin/env python3
"""ORBextractor::ComputePyramid timing on 752 x 480 images, 8 levels at 1.2 -- one frame per call, the stereo pair, a batch of 64:
  (a) osh_orb_pyramid_build without and with the download of the bordered levels;
  (b) the build without download followed by osh_orb_fast_detect_resident on its tokens;
  (c) osh_orb_fast_detect on host pyramids of the same frames (the same pixels, built beforehand by osh_host_orb_pyramid_cpu): the
      path before the build existed, with the same three detector kernels;
  (d) osh_host_orb_pyramid_cpu, the same statements (csrc/orb_pyramid.h) compiled for the host at the library's optimisation level
      on one thread of the same machine (with the bordered levels, as the reference's ComputePyramid leaves them);
  (e) operator() of the stand-in class end to end (one frame).
(b) against (c) in the same run is the comparison that decides.  The device calls are also split into staging, upload, kernels and
download by their own phase clocks (osh_orb_set_profiling on, which synchronises between the phases); every timed call ends in the
call's own stream synchronisation.  --warmup calls first, then --reps timed calls, median and spread (max - min) in ms.  The result
arrays are sized once, as a caller that keeps its buffers does.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/pyramid_timing.py --reps 50"""
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

import pyramid_numpy as pn  # noqa: E402
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
        print(f"{what:<66} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    inv = np.asarray(pn.standin_inv_scale(8), np.float32)
    distinct = [dict(image=np.ascontiguousarray(sf.make_image(900 + k, 480, 752)), inv_scale=inv, border=19) for k in range(4)]
    built, _ = orb.pyramid_cpu(distinct)      # the host pyramids of (c)
    host_frames = [sf.FastFrame(tuple(np.ascontiguousarray(lv) for lv in b["levels"]), 20, 7) for b in built]
    pn.assert_same(built[0], dict(zip(("levels", "bordered"), pn.build(distinct[0]["image"], inv, 19))), "the host pyramid")
    with orb.OrbMatcher(0) as m:
        for batch in (int(b) for b in a.batches.split(",")):
            items = [distinct[k % len(distinct)] for k in range(batch)]
            frames = [host_frames[k % len(distinct)] for k in range(batch)]
            name = f"{batch} x 752x480x8"
            sized = m.fast_detect(frames)
            caps = [(r["n_out"], r["n_cells"]) for r in sized]
            pf, pr, _pkeep, _pouts = orb.pyramid_args(items, download=False)
            df, dr, _dkeep, douts = orb.pyramid_args(items, download=True)
            rf, rr, _rkeep, routs = orb.fast_resident_args([dict(token=0, n_levels=8, ini_th=20, min_th=7)] * batch, caps)
            cf, cr, _ckeep, couts = orb.fast_args(frames, caps)

            def build():
                capi.check(lib.osh_orb_pyramid_build(m.ctx, batch, pf, pr), "osh_orb_pyramid_build", lib)

            def build_download():
                capi.check(lib.osh_orb_pyramid_build(m.ctx, batch, df, dr), "osh_orb_pyramid_build", lib)

            def build_detect():
                build()
                for j in range(batch):
                    rf[j].pyramid_token = pr[j].pyramid_token
                capi.check(lib.osh_orb_fast_detect_resident(m.ctx, batch, rf, rr), "osh_orb_fast_detect_resident", lib)

            def detect():
                capi.check(lib.osh_orb_fast_detect(m.ctx, batch, cf, cr), "osh_orb_fast_detect", lib)

            image_bytes = sum(it["image"].size for it in items)
            pyramid_bytes = sum(p.size for f in frames for p in f.pyramid)
            ms, sp = timed(build, a.reps, a.warmup)
            row(f"{name}: (a) osh_orb_pyramid_build", ms, sp, upload_bytes=image_bytes, frames_per_s=batch * 1e3 / ms)
            ms, sp = timed(build_download, a.reps, a.warmup)
            row(f"{name}: (a) osh_orb_pyramid_build with the download", ms, sp, frames_per_s=batch * 1e3 / ms)
            for g, e in zip(orb._pyramid_outputs(dr, douts)[:len(distinct)], built):
                for x, y in zip(g["bordered"], e["bordered"]):
                    assert np.array_equal(x, y), "the device pyramid differs from the host build"
            ms_b, sp_b = timed(build_detect, a.reps, a.warmup)
            row(f"{name}: (b) build + osh_orb_fast_detect_resident", ms_b, sp_b, upload_bytes=image_bytes, frames_per_s=batch * 1e3 / ms_b)
            ms_c, sp_c = timed(detect, a.reps, a.warmup)
            row(f"{name}: (c) osh_orb_fast_detect on host pyramids", ms_c, sp_c, upload_bytes=pyramid_bytes, frames_per_s=batch * 1e3 / ms_c)
            print(f"  (b) - (c) = {ms_b - ms_c:+.4f} ms; sum of the two spreads {sp_b + sp_c:.4f} ms", flush=True)
            rows.append(dict(what=f"{name}: (b) - (c)", ms=ms_b - ms_c, spread_ms=sp_b + sp_c))
            got, ref = orb._fast_outputs(rr, routs), orb._fast_outputs(cr, couts)
            for g, e in zip(got, ref):
                for key in ("level_count", "xy", "response", "level", "cell", "used_min_th"):
                    assert np.array_equal(g[key], e[key]), f"{name}: resident detector differs in {key}"
            m.set_profiling(True)
            ph_build, ph_res, ph_det = [], [], []
            for k in range(a.warmup + a.reps):
                build_detect()
                if k >= a.warmup:
                    ph_build.append(m.pyramid_times())
                    ph_res.append(m.fast_times())
            for k in range(a.warmup + a.reps):
                detect()
                if k >= a.warmup:
                    ph_det.append(m.fast_times())
            m.set_profiling(False)
            for label, ph in (("(b) build", np.array(ph_build)), ("(b) detect_resident", np.array(ph_res)), ("(c) detect", np.array(ph_det))):
                for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                    row(f"{name}:   {label} {phase}", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
            if batch > 2:
                continue     # the CPU row scales with the number of frames
            hf, hr, _hkeep, _houts = orb.pyramid_args(items, download=True)
            inner = C.c_double(0)

            def cpu():
                if host.osh_host_orb_pyramid_cpu(batch, hf, hr, C.byref(inner)) != 0:
                    raise RuntimeError("osh_host_orb_pyramid_cpu")
            cms, csp = timed(cpu, a.cpu_reps, 1)
            row(f"{name}: (d) CPU, one thread, osh_host_orb_pyramid_cpu", cms, csp, frames_per_s=batch * 1e3 / cms)
        ts = [orb.extract(distinct[0]["image"], nfeatures=1000, nlevels=8)["call_ms"] for _ in range(a.warmup + 20)][a.warmup:]
        row("1 x 752x480x8: (e) operator() of the stand-in class", float(np.median(ts)), float(max(ts) - min(ts)))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
