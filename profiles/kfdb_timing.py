#!/usr/bin/env python3
"""KeyFrameDatabase query timing: osh_orb_bow_db_query against databases of 1 000, 4 000 and 16 000 keyframes of about 1 200 words each
over a 10^6-word id space (synth_kfdb.make_trajectory: neighbouring keyframes share most of their words, distant ones few, with a
revisit now and then), for one query per call and for a batch of 64, split into staging, upload, kernels and download + write-back
by the call's own phase clocks (osh_orb_set_profiling on, which synchronises between the phases), the same calls unprofiled, and
DetectNBestCandidates of the single-thread C++ restatement of the test library (the reference's std::vector<std::list<KeyFrame*>>
inverted file) on the same host for the same queries.  The queries are the keyframes that continue the trajectory.  --warmup calls
first, then --reps timed calls, median and spread (max - min) in ms.  --json writes the rows."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import kfdb_numpy as kn  # noqa: E402
from orb_slam3_study_kr_amd import capi, host, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_kfdb as sk  # noqa: E402

N_WORDS = 1_000_000


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def cpu_baseline(vectors, n_kf, n_queries, reps):
    """DetectNBestCandidates of the C++ restatement for the first n_queries query keyframes, all database keyframes in one map and
    none connected; ms per query, median over `reps` runs of the script (each builds its own inverted file, which is not timed)."""
    n = n_kf + n_queries
    g = sk.KfdbGraph(N_WORDS, kf_id=list(range(1, n + 1)), kf_map=[0] * n, kf_bad=[0] * n, bow=vectors[:n], cov=[[] for _ in range(n)],
                     con=[[] for _ in range(n)], map_bad=[0])
    ops = [(sk.ADD, k, 0) for k in range(n_kf)] + [(sk.NBEST, n_kf + q, 3) for q in range(n_queries)]
    ms = [host.kfdb_restatement(g, ops)[1] / n_queries for _ in range(reps)]
    return float(np.median(ms)), float(max(ms) - min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,4000,16000")
    ap.add_argument("--words", type=int, default=1200)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cpu-queries", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    rows = []
    for n_kf in [int(v) for v in a.sizes.split(",") if v]:
        vectors = sk.make_trajectory(900 + n_kf, n_kf + a.batch, N_WORDS, a.words)
        queries = vectors[n_kf:]
        cpu_ms, cpu_spread = cpu_baseline(vectors, n_kf, a.cpu_queries, a.cpu_reps)
        rows.append(dict(what=f"{n_kf} keyframes, C++ restatement, one thread, one query", ms=cpu_ms, spread_ms=cpu_spread))
        print(f"{n_kf:6d} keyframes, C++ restatement 1 thread, per query   {cpu_ms:8.3f} ms  +- {cpu_spread:.3f}", flush=True)
        with orb.BowDb(N_WORDS) as db, orb.OrbMatcher(0) as m:
            t0 = time.perf_counter()
            handles = [db.add(w, v) for w, v in vectors[:n_kf]]
            add_ms = (time.perf_counter() - t0) * 1e3 / n_kf
            rows.append(dict(what=f"{n_kf} keyframes, osh_bow_db_add per keyframe", ms=add_ms, spread_ms=0.0))
            print(f"{n_kf:6d} keyframes, osh_bow_db_add per keyframe            {add_ms:8.3f} ms   {db.info()}", flush=True)
            if n_kf <= 1000:   # the model is a Python loop over the rows
                got = m.bow_db_query(db, queries[:2])
                for k in range(2):
                    kn.assert_same_query(got[k], kn.db_query(list(zip(handles, *zip(*vectors[:n_kf]))), *queries[k]), f"query {k}")
            for nb in (1, a.batch):
                cq, cr, keep, outs = orb.bow_db_args(queries[:nb], n_kf)

                def call():
                    capi.check(lib.osh_orb_bow_db_query(m.ctx, db.handle, nb, cq, cr), "osh_orb_bow_db_query", lib)
                reps = a.reps if nb == 1 else max(10, a.reps // 5)
                med, spread = timed(call, reps, a.warmup)
                listed = float(np.mean([int(o["n_rows"][0]) for o in outs]))
                scored = float(np.mean([int(np.sum(o["scored"][:int(o["n_rows"][0])])) for o in outs]))
                label = f"{n_kf} keyframes, batch of {nb}"
                rows.append(dict(what=f"{label}, one call", ms=med, spread_ms=spread, queries_per_s=nb * 1e3 / med, listed=listed, scored=scored))
                print(f"{label:<34} one call   {med:8.3f} ms  +- {spread:.3f}   {nb * 1e3 / med:9.1f} queries/s   listed {listed:.0f} scored {scored:.0f}")
                m.set_profiling(True)
                phases = []
                for k in range(a.warmup + reps):
                    call()
                    if k >= a.warmup:
                        phases.append(m.bow_db_times())
                m.set_profiling(False)
                phases = np.array(phases)
                for k, name in enumerate(("staging", "upload", "kernels", "download")):
                    pm, ps = float(np.median(phases[:, k])), float(phases[:, k].max() - phases[:, k].min())
                    rows.append(dict(what=f"{label}, {name}", ms=pm, spread_ms=ps))
                    print(f"{label:<34} {name:<10} {pm:8.3f} ms  +- {ps:.3f}", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
