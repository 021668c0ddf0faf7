#!/usr/bin/env python3
"""Optimizer::OptimizeSim3 timing: osh_sim3_optimize alone (staging, copies, one kernel launch, read-back) for batches of 1 / 16 /
64 problems, and one call through the reference signature (osh_host_optimize_sim3: stand-in keyframes + pair walk + device call +
write-back), at 50 / 300 / 1000 pairs with free and fixed scale (20 % swapped matches).  Every timed call ends in the call's own
stream synchronisation; --warmup calls first, then --reps timed calls, median and spread (max - min) in ms.  --json writes the rows."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from orb_slam3_study_kr_amd import capi  # noqa: E402
from orb_slam3_study_kr_amd import synth_sim3 as ss  # noqa: E402
from orb_slam3_study_kr_amd.lba import LbaSolver  # noqa: E402


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
    ap.add_argument("--pairs", default="50,300,1000")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    host = capi.load_host_library()
    rows = []
    print(f"{'pairs':>5} {'scale':>5} {'batch':>5} | {'device ms':>9} {'+-':>6} {'us/problem':>10} | {'host ms':>8} {'+-':>6} | it  n_in")
    with LbaSolver(0) as solver:
        for n in [int(v) for v in a.pairs.split(",")]:
            for fs in (False, True):
                for nb in [int(v) for v in a.batches.split(",")]:
                    cases = [ss.make_case(1000 + 97 * k + n, n, 0.2, fix_scale=fs) for k in range(nb)]
                    packs = [ss.pack(c) for c in cases]
                    keep = []
                    probs = (capi.Sim3Problem * nb)(*[ss.problem(p, keep) for p in packs])
                    rs = (capi.Sim3Result * nb)()
                    arrs = []
                    for k, p in enumerate(packs):
                        r, ar = ss.bind_result(len(p["index"]))
                        rs[k] = r
                        arrs.append(ar)

                    def dev():
                        capi.check(lib.osh_sim3_optimize(solver.ctx, nb, probs, rs), "osh_sim3_optimize", lib)
                    med, spread = timed(dev, a.reps, a.warmup)
                    row = dict(pairs=n, fix_scale=fs, batch=nb, device_ms=med, device_spread_ms=spread, us_per_problem=med * 1e3 / nb,
                               iterations=list(rs[0].iterations), n_in=rs[0].n_in)
                    hs = ""
                    if nb == 1:
                        inp = ss.host_input(cases[0])
                        nulled = np.zeros(len(cases[0].matches1), np.uint8)
                        S = np.zeros(8)
                        H = np.zeros(49)

                        def hostcall():
                            host.osh_host_optimize_sim3(C.byref(inp), capi.ptr(nulled, capi.c_uint8_p), capi.ptr(S, capi.c_double_p),
                                                        capi.ptr(H, capi.c_double_p))
                        hm, hsp = timed(hostcall, a.reps, a.warmup)
                        row.update(host_ms=hm, host_spread_ms=hsp)
                        hs = f"{hm:8.3f} {hsp:6.3f}"
                    rows.append(row)
                    print(f"{n:5d} {'fixed' if fs else 'free':>5} {nb:5d} | {med:9.3f} {spread:6.3f} {med * 1e3 / nb:10.1f} | {hs:>15} | "
                          f"{rs[0].iterations[0]},{rs[0].iterations[1]} {rs[0].n_in}", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
