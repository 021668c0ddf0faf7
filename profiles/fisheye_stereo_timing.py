#!/usr/bin/env python3
"""Frame::ComputeStereoFishEyeMatches timing: osh_orb_fisheye_stereo_match on one 512x512 rig frame with 1000 + 1000 keypoints inside
the overlap, split into staging, upload, kernels and download by the call's own phase clocks (osh_orb_set_profiling on, which
synchronises between the phases), the same call unprofiled, a batch of 64 such frames, and on one CPU thread of the same host the
brute-force part alone (the oracle's C distance matrix plus numpy's two-smallest selection) and the whole numpy restatement, named as
such.  Every timed call ends in the call's own stream synchronisation; --warmup calls first, then --reps timed calls, median and
spread (max - min) in ms.  --json writes the rows.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/fisheye_stereo_timing.py --batch 0 --reps 50"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import fisheye_stereo_numpy as fn  # noqa: E402
from oracle import binding as ob  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_fisheye as sf  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<52} {ms:9.3f} ms  +- {spread:.3f}", flush=True)
    distinct = [sf.make_fisheye_frame(500 + k, n_left=1000, n_right=1000, mono_left=0, mono_right=0) for k in range(8)]
    fr = distinct[0]
    with orb.OrbMatcher(0) as m:
        cf, cr, keep, outs = orb.fisheye_stereo_args([fr], True)

        def one():
            capi.check(lib.osh_orb_fisheye_stereo_match(m.ctx, 1, cf, cr), "osh_orb_fisheye_stereo_match", lib)
        row("single frame, one call", *timed(one, a.reps, a.warmup))
        exp = fn.compute(fr)
        fn.assert_matches(outs[0], exp, what="timed frame")
        print(f"  ({int(exp['ratio_ok'].sum())} ratio-accepted, {int((exp['stage'] == capi.OSH_FSTEREO_ACCEPTED).sum())} accepted of 1000)")
        m.set_profiling(True)
        phases = []
        for k in range(a.warmup + a.reps):
            one()
            if k >= a.warmup:
                phases.append(m.fisheye_stereo_times())
        m.set_profiling(False)
        phases = np.array(phases)
        for k, name in enumerate(("staging", "upload", "kernels", "download")):
            row(f"single frame, {name}", float(np.median(phases[:, k])), float(phases[:, k].max() - phases[:, k].min()))
        if a.batch:
            frames = [distinct[k % len(distinct)] for k in range(a.batch)]
            bf_, br_, bkeep, bouts = orb.fisheye_stereo_args(frames, False)

            def batch():
                capi.check(lib.osh_orb_fisheye_stereo_match(m.ctx, a.batch, bf_, br_), "osh_orb_fisheye_stereo_match", lib)
            reps = max(20, a.reps // 8)
            bm, bs = timed(batch, reps, 3)
            row(f"batch of {a.batch} frames ({reps} reps)", bm, bs, frames_per_s=a.batch * 1e3 / bm)
            print(f"  {a.batch * 1e3 / bm:.1f} frames/s, {bm / a.batch:.4f} ms per frame")

    def brute():
        d = ob.distance_matrix(fr.left_desc, fr.right_desc)
        two = np.partition(d, 1, axis=1)[:, :2]
        return d.argmin(axis=1), two
    row("CPU, one thread: C distance matrix + numpy 2-smallest", *timed(brute, max(5, a.reps // 10), 2))
    row("CPU, one thread: numpy restatement (whole function)", *timed(lambda: fn.compute(fr), 3, 1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
