#!/usr/bin/env python3
"""4-DoF pose graph (Optimizer::OptimizeEssentialGraph4DoF) timing: osh_pgo4_solve at 100 / 500 / 1000 / 4000 keyframes of a
synthetic inertial loop, one loop closure and two (an earlier loop edge pair on top).  The method of pgo_timing.py: one
warm-up call per case, then 5 timed calls, each ended by the call's own read-back; median and spread (max - min) in ms, with LM
iterations, trials and the envelope size.  --sizes / --reps narrow the run; --json writes the rows."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles"))

from orb_slam3_study_kr_amd import synth_pgo as sp  # noqa: E402
from orb_slam3_study_kr_amd.pgo import PgoSolver  # noqa: E402
from pgo_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,500,1000,4000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    print(f"{'KFs':>5} {'loops':>5} {'edges':>6} | {'solve ms':>9} {'+-':>6} | it  tr | env entries  tiles tall")
    with PgoSolver(0) as s:
        for n in [int(x) for x in a.sizes.split(",")]:
            for loops in (1, 2):
                m = sp.make_inertial_loop(n, seed=7, earlier_loop=loops == 2, rp_noise=0.001)
                g, _, _ = sp.pack_loop4(m)
                r, med, spread = timed(lambda: s.solve4(g), a.reps)
                row = dict(kfs=n, loops=loops, edges=int(len(g.edge_ij)), solve_ms=med, solve_spread_ms=spread, iterations=r.iterations,
                           trials=r.trials, envelope_entries=int(r.envelope_entries), envelope_tiles=r.envelope_tiles, tall_columns=r.tall_columns)
                rows.append(row)
                print(f"{n:5d} {loops:5d} {row['edges']:6d} | {med:9.2f} {spread:6.2f} | {r.iterations:2d} {r.trials:3d} | "
                      f"{row['envelope_entries']:11d} {r.envelope_tiles:6d} {r.tall_columns:4d}", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
