#!/usr/bin/env python3
"""Sim3 pose graph (Optimizer::OptimizeEssentialGraph) timing: osh_pgo_solve alone and the full host call (graph walk + solve +
write-back through the reference signature) at 100 / 500 / 1000 / 4000 keyframes, one loop closure and two (an earlier loop
edge pair on top).  One warm-up call per case, then 5 timed calls, each ended by the call's own synchronisation (osh_pgo_solve
reads its result back; the host call returns after the write-back); median and spread (max - min) in ms, with LM iterations,
trials and the envelope size.  --sizes / --reps narrow the run; --json writes the rows."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from orb_slam3_study_kr_amd import synth_pgo as sp  # noqa: E402
from orb_slam3_study_kr_amd.pgo import PgoSolver  # noqa: E402


def timed(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(ts)), float(max(ts) - min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,500,1000,4000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    rows = []
    print(f"{'KFs':>5} {'loops':>5} {'edges':>6} | {'solve ms':>9} {'+-':>6} | {'host ms':>9} {'+-':>6} | it  tr | env entries  tiles tall")
    with PgoSolver(0) as s:
        for n in [int(x) for x in a.sizes.split(",")]:
            for loops in (1, 2):
                m = sp.make_map(n, seed=7, mono=True, earlier_loop=loops == 2, band=6)
                g, _, _ = sp.pack_loop(m)
                r, med, spread = timed(lambda: s.solve(g), a.reps)
                row = dict(kfs=n, loops=loops, edges=int(len(g.edge_ij)), solve_ms=med, solve_spread_ms=spread, iterations=r.iterations,
                           trials=r.trials, envelope_entries=int(r.envelope_entries), envelope_tiles=r.envelope_tiles, tall_columns=r.tall_columns)
                hmed = hspread = float("nan")
                if not a.no_host:
                    hts = []
                    for k in range(a.reps + 1):
                        with sp.HostPgoMap(m) as h:   # a fresh map per call: the call moves it
                            h.run()
                            if k:
                                hts.append(h.lib.osh_host_last_call_ms())
                    hmed, hspread = float(np.median(hts)), float(max(hts) - min(hts))
                row.update(host_ms=hmed, host_spread_ms=hspread)
                rows.append(row)
                print(f"{n:5d} {loops:5d} {row['edges']:6d} | {med:9.2f} {spread:6.2f} | {hmed:9.2f} {hspread:6.2f} | "
                      f"{r.iterations:2d} {r.trials:3d} | {row['envelope_entries']:11d} {r.envelope_tiles:6d} {r.tall_columns:4d}", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
