#!/usr/bin/env python3
"""The image front end (remap, then grey) on 752 x 480 images, 8 levels at 1.2 -- one frame per call, the stereo pair, a batch of
64, for a grey source with a rectify map and for a BGR source with a rectify map:
  (a) osh_orb_prepare alone without and with the download of the grey image, and its kernel share (its own phase clock);
  (b) osh_orb_extract_raw: only the raw image goes up;
  (c) the way to the same keypoints before the stage existed: csrc/orb_prepare.h compiled for the host at the library's optimisation
      level on one thread of the same machine (osh_host_orb_prepare_cpu), followed by osh_orb_extract on its image.  The CPU row is
      this repository's own statements, not OpenCV's SIMD code, which cannot be built here;
  (d) osh_orb_extract alone on ready images: what the stage adds is (b) - (d).
(b), (c) and (d) alternate inside one loop, so they see the same machine.  Every timed call ends in the call's own stream
synchronisation.  --warmup rounds first, then --reps timed rounds, median and spread (max - min) in ms.  The result arrays are sized
once, as a caller that keeps its buffers does.  (b) and (c) are checked to give the same keypoints.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/prepare_timing.py --reps 50"""
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
import prepare_numpy as pp  # noqa: E402
import pyramid_numpy as pn  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_fast as sf  # noqa: E402

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="1,2,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    rows = []

    def row(what, ts, **kw):
        ms, spread = float(np.median(ts)), float(max(ts) - min(ts))
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<78} {ms:9.4f} ms  +- {spread:.4f}", flush=True)
        return ms

    nl = 8
    scale = [F(1)]
    for _ in range(1, nl):
        scale.append(F(scale[-1] * F(1.2)))
    keys = dict(inv_scale=np.asarray(pn.standin_inv_scale(nl), F), scale=np.asarray(scale, F),
                n_features=np.asarray(on.features_per_level(1000, 1.2, nl), np.int32), pattern=orb.standin_pattern(), ini_th=20, min_th=7, border=19)
    mx, my = pp.rectify_maps(480, 752, (480, 752), f=0.61, shift=(4.3, -2.6), zoom=1.0)
    grey = [np.ascontiguousarray(sf.make_image(900 + k, 480, 752)) for k in range(4)]
    bgr = [np.ascontiguousarray(np.stack([sf.make_image(900 + k + 10 * c, 480, 752) for c in range(3)], -1)) for k in range(4)]
    with orb.OrbMatcher(0) as m, m.rectify_map(mx, my, (480, 752)) as rmap:
        for kind, images in (("grey + remap", grey), ("BGR + remap", bgr)):
            for batch in (int(b) for b in a.batches.split(",")):
                name = f"{batch} x 752x480 {kind}"
                items = [dict(image=images[k % 4], order="bgr", map=rmap, **keys) for k in range(batch)]
                raw_bytes = sum(it["image"].size for it in items)
                # the CPU front end once, for the ready images of (d) and the check of (c)
                ready, _ = orb.prepare_cpu(items[:min(batch, 4)])
                ready = [np.ascontiguousarray(r["gray"]) for r in ready]
                ready_items = [dict(it, image=ready[k % 4]) for k, it in enumerate(items)]
                caps = [r["n_out"] for r in m.extract(ready_items, [0] * batch)]
                pf0, pr0, *_ = orb.prepare_args(items, False)
                pf1, pr1, _m1, _k1, pouts = orb.prepare_args(items, True)
                rf, rr, _rk, routs = orb.extract_raw_args(items, caps)
                hf, hr, hmaps, _hk, houts = orb.prepare_args(items, True)
                for k in range(batch):
                    hf[k].map = None
                cf, cr, _ck, couts = orb.extract_args([dict(it, image=o["gray_whole"][:, :752]) for it, o in zip(items, houts)], caps)
                df, dr, _dk, douts = orb.extract_args(ready_items, caps)

                def prepare():
                    capi.check(lib.osh_orb_prepare(m.ctx, batch, pf0, pr0), "osh_orb_prepare", lib)

                def prepare_download():
                    capi.check(lib.osh_orb_prepare(m.ctx, batch, pf1, pr1), "osh_orb_prepare", lib)

                def raw():
                    capi.check(lib.osh_orb_extract_raw(m.ctx, batch, pf0, rf, rr, None), "osh_orb_extract_raw", lib)

                def cpu_then_extract():
                    t0 = time.perf_counter()
                    if host.osh_host_orb_prepare_cpu(batch, hf, hmaps, hr, None) != 0:
                        raise RuntimeError("osh_host_orb_prepare_cpu")
                    t1 = time.perf_counter()
                    capi.check(lib.osh_orb_extract(m.ctx, batch, cf, cr), "osh_orb_extract", lib)
                    return (t1 - t0) * 1e3

                def extract():
                    capi.check(lib.osh_orb_extract(m.ctx, batch, df, dr), "osh_orb_extract", lib)

                def clock(fn_):
                    t0 = time.perf_counter()
                    out = fn_()
                    return (time.perf_counter() - t0) * 1e3, out

                t = dict(a0=[], a1=[], b=[], c=[], c_cpu=[], d=[])
                for k in range(a.warmup + a.reps):
                    keep = k >= a.warmup
                    for key, fn_ in (("a0", prepare), ("a1", prepare_download), ("b", raw), ("c", cpu_then_extract), ("d", extract)):
                        ms, out = clock(fn_)
                        if keep:
                            t[key].append(ms)
                            if key == "c":
                                t["c_cpu"].append(out)
                for o, r in zip(pouts[:4], ready):
                    assert np.array_equal(o["gray"], r), f"{name}: the device image differs from the host build"
                got, ref = orb._extract_outputs(rr, routs), orb._extract_outputs(cr, couts)
                for g, e in zip(got, ref):
                    assert g["n_out"] == e["n_out"] > 500, (g["n_out"], e["n_out"])
                    for key in ("level_count", "xy", "level", "response", "angle", "size", "descriptors"):
                        assert np.array_equal(g[key], e[key]), f"{name}: extract_raw differs in {key}"
                row(f"{name}: (a) osh_orb_prepare", t["a0"], upload_bytes=raw_bytes, frames_per_s=batch * 1e3 / np.median(t["a0"]))
                row(f"{name}: (a) osh_orb_prepare with the download", t["a1"])
                ms_b = row(f"{name}: (b) osh_orb_extract_raw", t["b"], upload_bytes=raw_bytes, frames_per_s=batch * 1e3 / np.median(t["b"]))
                ms_c = row(f"{name}: (c) CPU front end, one thread, then osh_orb_extract", t["c"], frames_per_s=batch * 1e3 / np.median(t["c"]))
                row(f"{name}:   (c) of which the CPU front end", t["c_cpu"])
                ms_d = row(f"{name}: (d) osh_orb_extract on ready images", t["d"], upload_bytes=batch * 480 * 752, frames_per_s=batch * 1e3 / np.median(t["d"]))
                print(f"  (b) - (d) = {ms_b - ms_d:+.4f} ms (what the stage adds); (c) - (b) = {ms_c - ms_b:+.4f} ms", flush=True)
                rows.append(dict(what=f"{name}: (b) - (d)", ms=ms_b - ms_d))
                rows.append(dict(what=f"{name}: (c) - (b)", ms=ms_c - ms_b))
                m.set_profiling(True)
                ph = []
                for k in range(a.warmup + a.reps):
                    prepare_download()
                    if k >= a.warmup:
                        ph.append(m.prepare_times())
                m.set_profiling(False)
                ph = np.array(ph)
                for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                    row(f"{name}:   (a) with the download: {phase}", ph[:, k])
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
