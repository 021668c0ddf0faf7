#!/usr/bin/env python3
"""ORBextractor::operator() in one device call, on 752 x 480 frames, 8 levels at 1.2, nfeatures 1000:
  (a) osh_orb_octree_distribute alone on the FAST candidates of such frames (the eight lists of one frame per call, of the stereo
      pair, of 64 frames), one workgroup per (frame, level) list, the candidates coming from the host;
  (b) osh_host_orb_octree_cpu, the same statements (csrc/orb_octree.h) compiled for the host at the library's optimisation level on
      one thread of the same machine;
  (c) operator() of the stand-in class end to end (one frame): ComputePyramid, ComputeKeyPointsOctTree with the host octree and
      its two round trips, osh_orb_describe.  Nothing on this path changed, so this is also the figure of the commit before;
  (d) ORBextractor::ExtractBatch of one frame, with and without bKeepPyramid;
  (e) the stereo pair: ExtractBatch of two frames as one call against two operator() calls;
  (f) osh_orb_extract on 1, 2 and 64 frames without the download of the levels, with its four times (pyramid, detector, quadtree,
      orientation + descriptors + download) from osh_orb_extract_get_times.
The device calls are also split by their own phase clocks (osh_orb_set_profiling on, which synchronises between the phases); every
timed call ends in the call's own stream synchronisation.  --warmup calls first, then --reps timed calls, median and spread
(max - min) in ms.  The result arrays are sized once, as a caller that keeps its buffers does.  The device octree is checked against
the host build before anything is timed.  (c), (d) and (e) are the wall times of the member calls alone, measured inside the test
library.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/extract_timing.py --reps 50"""
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

import octree_numpy as on  # noqa: E402
import pyramid_numpy as pn  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import host as hostpy  # noqa: E402
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
    ap.add_argument("--cpu-reps", type=int, default=20)
    ap.add_argument("--batches", default="1,2,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<66} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    per_level = on.features_per_level(1000, 1.2, 8)
    frames = [sf.make_frame(31 + k, 752, 480, 8) for k in range(4)]
    with orb.OrbMatcher(0) as m:
        detected = m.fast_detect(frames)
        frame_lists = []
        for fr, d in zip(frames, detected):
            lists = []
            for l, im in enumerate(fr.pyramid):
                sel = d["level"] == l
                lists.append((np.ascontiguousarray(d["xy"][sel]), np.ascontiguousarray(d["response"][sel]), im.shape[1] - 32, im.shape[0] - 32, per_level[l]))
            frame_lists.append(lists)
        print("candidates per level of frame 0:", [len(l[1]) for l in frame_lists[0]], "N per level:", per_level, flush=True)
        for batch in (int(b) for b in a.batches.split(",")):
            lists = [l for k in range(batch) for l in frame_lists[k % len(frame_lists)]]
            name = f"{batch} x 752x480x8 ({len(lists)} lists, {sum(len(l[1]) for l in lists)} candidates)"
            cl, cr, _keep, outs = orb.octree_args(lists)
            hl, hr, _hkeep, houts = orb.octree_args(lists)
            inner = C.c_double(0)

            def device():
                capi.check(lib.osh_orb_octree_distribute(m.ctx, len(lists), cl, cr), "osh_orb_octree_distribute", lib)

            def cpu():
                if host.osh_host_orb_octree_cpu(len(lists), hl, hr, C.byref(inner)) != 0:
                    raise RuntimeError("osh_host_orb_octree_cpu")

            device()
            cpu()
            for g, e in zip(orb._octree_outputs(cr, outs), orb._octree_outputs(hr, houts)):
                assert g["n_out"] == e["n_out"] and np.array_equal(g["index"], e["index"]), "the device octree differs from the host build"
            kept = sum(int(cr[k].n_out) for k in range(len(lists)))
            ms, sp = timed(device, a.reps, a.warmup)
            row(f"{name}: (a) osh_orb_octree_distribute", ms, sp, kept=kept, frames_per_s=batch * 1e3 / ms)
            m.set_profiling(True)
            ph = []
            for k in range(a.warmup + a.reps):
                device()
                if k >= a.warmup:
                    ph.append(m.octree_times())
            m.set_profiling(False)
            ph = np.array(ph)
            for k, phase in enumerate(("staging", "upload", "kernel", "download")):
                row(f"{name}:   (a) {phase}", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
            cms, csp = timed(cpu, a.cpu_reps if batch <= 2 else max(a.cpu_reps // 4, 3), 1)
            row(f"{name}: (b) CPU, one thread, osh_host_orb_octree_cpu", cms, csp, frames_per_s=batch * 1e3 / cms)
        images = [np.ascontiguousarray(sf.make_image(900 + k, 480, 752)) for k in range(4)]

        def member(fn_):
            ts = [fn_() for _ in range(a.warmup + a.reps)][a.warmup:]
            return float(np.median(ts)), float(max(ts) - min(ts))

        ms_c, sp_c = member(lambda: orb.extract(images[0], nfeatures=1000, nlevels=8)["call_ms"])
        row("1 x 752x480x8: (c) operator() of the stand-in class", ms_c, sp_c)
        for keep in (True, False):
            ms_d, sp_d = member(lambda: hostpy.orbextractor_extract_batch(images[:1], [(0, 0)], keep_pyramid=keep)[0]["call_ms"])
            row(f"1 x 752x480x8: (d) ExtractBatch, bKeepPyramid = {keep}", ms_d, sp_d)
            print(f"  (d) - (c) = {ms_d - ms_c:+.4f} ms; sum of the two spreads {sp_c + sp_d:.4f} ms", flush=True)
        ms_2, sp_2 = member(lambda: sum(orb.extract(im, nfeatures=1000, nlevels=8)["call_ms"] for im in images[:2]))
        row("2 x 752x480x8: (e) two operator() calls", ms_2, sp_2)
        ms_e, sp_e = member(lambda: hostpy.orbextractor_extract_batch(images[:2], [(0, 0)] * 2)[0]["call_ms"])
        row("2 x 752x480x8: (e) ExtractBatch of the pair, one call", ms_e, sp_e)
        scale = [np.float32(1)]
        for _ in range(7):
            scale.append(np.float32(scale[-1] * np.float32(1.2)))
        item = lambda im: dict(image=im, inv_scale=np.asarray(pn.standin_inv_scale(8), np.float32), scale=np.asarray(scale, np.float32),
                               n_features=np.asarray(per_level, np.int32), pattern=orb.standin_pattern())
        for batch in (int(b) for b in a.batches.split(",")):
            items = [item(images[k % len(images)]) for k in range(batch)]
            caps = [r["n_out"] for r in m.extract(items, [0] * batch)]
            ef, er, _ekeep, _eouts = orb.extract_args(items, caps)

            def fused():
                capi.check(lib.osh_orb_extract(m.ctx, batch, ef, er), "osh_orb_extract", lib)

            ms, sp = timed(fused, a.reps, a.warmup)
            row(f"{batch} x 752x480x8: (f) osh_orb_extract ({sum(caps)} keypoints)", ms, sp, frames_per_s=batch * 1e3 / ms)
            m.set_profiling(True)
            ph = []
            for k in range(a.warmup + a.reps):
                fused()
                if k >= a.warmup:
                    ph.append(m.extract_times())
            m.set_profiling(False)
            ph = np.array(ph)
            for k, phase in enumerate(("pyramid", "detector", "quadtree", "orientation, descriptors, download")):
                row(f"{batch} x 752x480x8:   (f) {phase}", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
