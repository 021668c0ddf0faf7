#!/usr/bin/env python3
"""KeyFrameCulling timing: LocalMapping::KeyFrameCulling's counting (src/LocalMapping.cc:976-1042) on one call with 30 and with 100
candidates of about 1000 slots each, at the observation lengths of synth_keyframe_cull.py, with 0 and with 2 culls in the call.

The device path is pack (PackKeyFrameCull on the stand-in map, host), stage (osh_orb_keyframe_cull_stage) and one
osh_orb_keyframe_cull_count per cull plus one; each is timed by wall clock unprofiled (stage and count end in a stream
synchronisation), and stage and count are split by the entry's phase clock (osh_orb_keyframe_cull_get_times under
osh_orb_set_profiling: packing the records, upload, mask + kernel, download).  It is set against
  * osh_host_keyframe_cull_cpu: the same header (csrc/keyframe_cull.h) on one thread over the packed records, and
  * the counting loop in the reference's shape on the same objects: per candidate and slot a copy of GetObservations() and a walk.
The sums of nMPs and nRedundantObservations of all three are compared before anything is timed, and the device counts equal the
header's bit for bit.  A cull costs the host paths a recount of the candidates after it; the rows "2 culls" recount from
candidates 1/3 and 2/3 down the list.  --warmup calls first, then --reps timed calls, median and spread (max - min) in ms.

Per-kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/keyframe_cull_timing.py --reps 50"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_keyframe_cull as sk  # noqa: E402
from orb_slam3_study_kr_amd.host import HostCullGraph  # noqa: E402


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
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--keyframes", type=int, default=400)
    ap.add_argument("--candidates", default="30,100")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    if lib.osh_device_count() < 1:
        raise SystemExit("keyframe_cull_timing: no HIP device visible")
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<72} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    n_max = max(int(c) for c in a.candidates.split(","))
    sc = sk.random_scene(n_max, a.slots, a.keyframes, seed=11)
    with HostCullGraph(sc) as g, orb.OrbMatcher(0) as m:
        for n_c in (int(c) for c in a.candidates.split(",")):
            cand = sc.covisible[:n_c]
            pk = g.pack(cand, objects=False)
            pb = sk.CullProblem(int(pk["obs_kf"].max()) + 1 if len(pk["obs_kf"]) else n_c, n_c, 0.9, pk["cand_slot_off"], pk["slot_point"], pk["slot_level"],
                                pk["point_n_obs"], pk["point_bad"], pk["point_obs_off"], pk["obs_kf"], pk["obs_level"], pk["obs_weight"])
            pb.n_keyframes = max(pb.n_keyframes, n_c)
            name = f"{n_c} candidates"
            culls = [n_c // 3, 2 * n_c // 3]
            sets = [([], 0), (culls[:1], culls[0] + 1), (culls, culls[1] + 1)]
            # equal first
            m.keyframe_cull_stage(pb)
            ref = g.pack_and_reference_times(cand)
            for removed, first in sets:
                dev, cpu = m.keyframe_cull_count(removed, first), orb.kfcull_cpu(pb, removed, first)[0]
                for k in dev:
                    assert np.array_equal(dev[k], cpu[k]), (name, k, removed)
                if not removed:
                    assert (int(dev["n_mps"].sum()), int(dev["n_redundant"].sum())) == (ref["n_mps"], ref["n_redundant"]), name
            lengths = np.diff(pb.point_obs_off)
            print(f"{name}: {len(pb.slot_point)} slots, {pb.n_points} distinct points, {len(pb.obs_kf)} observations (median run {int(np.median(lengths))}, "
                  f"mean {lengths.mean():.1f}, longest {lengths.max()}), table {pb.n_keyframes}", flush=True)

            host = [g.pack_and_reference_times(cand) for _ in range(a.host_reps)]
            pack = np.array([h["pack_ms"] for h in host]); loop = np.array([h["reference_loop_ms"] for h in host])
            row(f"{name}: pack (PackKeyFrameCull, host)", float(np.median(pack)), float(pack.max() - pack.min()))
            ms_stage, sp = timed(lambda: m.keyframe_cull_stage(pb), a.reps, a.warmup)
            row(f"{name}: stage (wall)", ms_stage, sp)
            counts = []
            for removed, first in sets:
                ms, sp = timed(lambda: m.keyframe_cull_count(removed, first), a.reps, a.warmup)
                counts.append(ms)
                row(f"{name}: count of candidates {first}.. under {len(removed)} removed (wall)", ms, sp)
            m.set_profiling(True)
            ph = []
            for k in range(a.warmup + a.reps):
                m.keyframe_cull_stage(pb)
                m.keyframe_cull_count([], 0)
                if k >= a.warmup:
                    ph.append(m.keyframe_cull_times())
            m.set_profiling(False)
            ph = np.array(ph)
            for k, phase in enumerate(("stage: records packed", "stage: upload", "count: mask + kernel", "count: download")):
                row(f"{name}:   {phase} (profiled)", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
            row(f"{name}: device path, 0 culls = pack + stage + 1 count", float(np.median(pack)) + ms_stage + counts[0], 0.0)
            row(f"{name}: device path, 2 culls = pack + stage + 3 counts", float(np.median(pack)) + ms_stage + sum(counts), 0.0)

            cpu_ms = []
            for removed, first in sets:
                t = np.array([orb.kfcull_cpu(pb, removed, first)[1] for _ in range(max(3, a.host_reps))])
                cpu_ms.append(float(np.median(t)))
                row(f"{name}: same header, one thread, candidates {first}.. ({len(removed)} removed)", cpu_ms[-1], float(t.max() - t.min()))
            row(f"{name}: same header, one thread, 0 culls = pack + 1 count", float(np.median(pack)) + cpu_ms[0], 0.0)
            row(f"{name}: same header, one thread, 2 culls = pack + 3 counts", float(np.median(pack)) + sum(cpu_ms), 0.0)
            row(f"{name}: reference-shaped loop on the objects, one pass, one thread", float(np.median(loop)), float(loop.max() - loop.min()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
