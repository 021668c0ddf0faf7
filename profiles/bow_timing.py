#!/usr/bin/env python3
"""TemplatedVocabulary::transform timing: osh_orb_bow_transform on a generated full 10-way, 6-level vocabulary (1 111 110 nodes
besides the root, 10^6 words, 35.6 MB of descriptors) and frames of 1 000, 2 000 and 4 000 descriptors, for one frame and for a
batch of 64, split into staging, upload, kernels and download + write-back by the call's own phase clocks (osh_orb_set_profiling
on, which synchronises between the phases), the same calls unprofiled, and the single-thread C++ restatement of the test library on
the same host.  --warmup calls first, then --reps timed calls, median and spread (max - min) in ms.  --json writes the rows."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bow_numpy as bn  # noqa: E402
from orb_slam3_study_kr_amd import capi, host, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_bow as sb  # noqa: E402


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
    ap.add_argument("--sizes", default="1000,2000,4000")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--levelsup", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    tree = sb.make_full_vocab(1)
    print(f"vocabulary: k = {tree.k}, L = {tree.L}, {tree.n} nodes, {int(tree.is_leaf.sum())} words")
    rows = []
    with orb.BowVocab(tree) as vocab, orb.OrbMatcher(0) as m:
        for n in [int(v) for v in a.sizes.split(",") if v]:
            distinct = [sb.random_features(700 + 10 * n + k, n) for k in range(8)]
            cpu = [host.bow_restatement(tree, distinct[0], a.levelsup, timed=True) for _ in range(a.cpu_reps)]
            exp, cpu_ms = cpu[0][0], [c[1] for c in cpu]
            rows.append(dict(what=f"{n} features, C++ restatement, one thread", ms=float(np.median(cpu_ms)), spread_ms=float(max(cpu_ms) - min(cpu_ms))))
            print(f"{n:5d} features, C++ restatement 1 thread      {np.median(cpu_ms):8.3f} ms  +- {max(cpu_ms) - min(cpu_ms):.3f}")
            for nb in (1, a.batch):
                frames = [distinct[k % len(distinct)] for k in range(nb)]
                cf, cr, keep, outs = orb.bow_args(frames, False)

                def call():
                    capi.check(lib.osh_orb_bow_transform(m.ctx, vocab.handle, a.levelsup, nb, cf, cr), "osh_orb_bow_transform", lib)
                reps = a.reps if nb == 1 else max(10, a.reps // 5)
                med, spread = timed(call, reps, a.warmup)
                bn.assert_same(orb.bow_trim(outs[0]), exp, f"{n} features, batch of {nb}", stages=False)
                label = f"{n} features, batch of {nb}"
                rows.append(dict(what=f"{label}, one call", ms=med, spread_ms=spread, frames_per_s=nb * 1e3 / med))
                print(f"{label:<32} one call   {med:8.3f} ms  +- {spread:.3f}   {nb * 1e3 / med:9.1f} frames/s")
                m.set_profiling(True)
                phases = []
                for k in range(a.warmup + reps):
                    call()
                    if k >= a.warmup:
                        phases.append(m.bow_times())
                m.set_profiling(False)
                phases = np.array(phases)
                for k, name in enumerate(("staging", "upload", "kernels", "download")):
                    pm, ps = float(np.median(phases[:, k])), float(phases[:, k].max() - phases[:, k].min())
                    rows.append(dict(what=f"{label}, {name}", ms=pm, spread_ms=ps))
                    print(f"{label:<32} {name:<10} {pm:8.3f} ms  +- {ps:.3f}", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
