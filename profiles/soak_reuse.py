#!/usr/bin/env python3
"""Does a result depend on what its context ran before?  ONE long-lived solver context takes a random sequence of calls of every kind and
size -- local-BA batches of 1 .. 200 windows (both packers, windows of 1 .. 60 keyframes, a 300-keyframe map through the global-memory
factorisation), LocalInertialBA windows alone and in batches, FullInertialBA-shaped maps in the dense and in the banded layout -- and
every result is compared, bit for bit, with the same call in a FRESH context (buffers that grow and are reused, sections a kernel
assumes to be zero, state left by the previous call).  Found in r03: the banded layout of an inertial map read 15 columns past the band it
had written (profiles/r03_soak.txt).  Pose, pose-inertial, both pose graphs and OptimizeSim3 batches join the draw through the raw calls
of tests/test_gpu_reuse.py (every result scalar and output array compared).  OSH_ZERO_NEW_BUFFERS=1: new allocations start zeroed, so
a fresh context never starts from memory the allocator recycled from the previous one.
Usage: python profiles/soak_reuse.py [seconds] [seed]"""
import dataclasses
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
os.environ["OSH_ZERO_NEW_BUFFERS"] = "1"

from orb_slam3_study_kr_amd import lba, synth  # noqa: E402
from orb_slam3_study_kr_amd import synth_inertial as si  # noqa: E402
import test_gpu_reuse as tr  # noqa: E402

LBA_FIELDS = ("pose_qt", "points", "edge_chi2", "chi2_trace")
LIBA_FIELDS = ("chi2_trace", "pose_twb", "vel", "bias_g", "bias_a", "points")


def same(a, b, fields):
    if a.iterations != b.iterations or a.trials != b.trials:
        return f"iterations {a.iterations}/{b.iterations} trials {a.trials}/{b.trials}"
    for f in fields:
        if not np.array_equal(getattr(a, f), getattr(b, f)):
            return f"{f}: max difference {np.abs(np.asarray(getattr(a, f), dtype=np.float64) - np.asarray(getattr(b, f), dtype=np.float64)).max():.3g}"
    return None


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 200.0
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 31)
    t_end = time.time() + seconds
    pool = {}

    def lba_window(k):
        if ("l", k) not in pool:
            r = np.random.default_rng(k)
            pool[("l", k)] = synth.make_window(3000 + k, n_free=int(r.choice([1, 3, 8, 20, 47, 60])), n_fixed=int(r.integers(1, 6)),
                                               n_points=int(r.choice([60, 400, 1500, 5000])), stereo=bool(r.random() < 0.7),
                                               track_len=(3, int(r.integers(5, 20))), obs_dropout=float(r.choice([0.0, 0.2])), max_iterations=int(r.choice([3, 6])))
        return pool[("l", k)]

    def inertial_window(k, n_opt=None):
        key = ("i", k, n_opt)
        if key not in pool:
            if n_opt is None:
                pool[key] = si.make_inertial_window(4000 + k, n_opt=int(np.random.default_rng(k).choice([4, 10, 14])), n_points=int(np.random.default_rng(k + 1).choice([600, 2000, 3600])))
            else:
                w = si.make_inertial_window(900 + n_opt, n_opt=n_opt, n_fixed=0, n_points=40 * n_opt, large=True)
                pool[key] = dataclasses.replace(w, lambda_init=1e-5, max_iterations=4, link_robust=np.ones_like(w.link_robust))
        return pool[key]

    def other_call(kind):
        k = int(rng.integers(0, 6))
        if kind == "pose":
            frames = [synth.make_pose_frame(60 + (k + i) % 6, n_points=[12, 300, 900, 1500][(k + i) % 4]) for i in range(int(rng.choice([1, 5, 48])))]
            return tr.pose_call(f"{len(frames)} frames", frames)
        if kind == "posei":
            ins = tr.posei_script_inputs()
            return tr.posei_call(f"set {k}", [ins["batch1"], ins["mode0"], ins["mixed"], [ins["large"]], [ins["recovery"]], ins["batch1"][:3]][k])
        if kind == "pgo":
            return tr.pgo_call(f"{[50, 300, 1000][k % 3]} vertices", tr._pgo_graph([50, 300, 1000][k % 3], mono=k < 3), dense=k == 5)
        if kind == "pgo4":
            return tr.pgo4_call(f"{[50, 300][k % 2]} vertices", tr._pgo4_graph([50, 300][k % 2]), dense=k == 4)
        ins = tr.sim3_script_inputs()
        return tr.sim3_call(f"set {k}", [ins["batch"], [ins["round2"]], [ins["early"]], [ins["kb8"]], [ins["pin"]], ins["batch"][:4]][k])

    n = 0
    kinds = {}
    with lba.LbaSolver(0) as live:
        while time.time() < t_end:
            kind = str(rng.choice(["lba_small", "lba_batch", "lba_map", "liba_one", "liba_batch", "liba_dense_map", "liba_banded_map",
                                   "pose", "posei", "pgo", "pgo4", "sim3"],
                                  p=[0.15, 0.12, 0.04, 0.1, 0.1, 0.07, 0.07, 0.07, 0.07, 0.07, 0.07, 0.07]))
            if kind in ("pose", "posei", "pgo", "pgo4", "sim3"):
                call = other_call(kind)
                got = call.run(live.lib, live.ctx)
                missing = call.written(got)
                ref = tr.fresh_run(live.lib, call)
                diff = next((f"{k}: {tr._first_difference(got[k], ref[k])}" for k in sorted(got) if got[k].tobytes() != ref[k].tobytes()), None)
                if missing or diff:
                    print(f"MISMATCH call {n} ({kind}: {call.desc}): {'; '.join(missing) or diff}", flush=True)
                    return 1
                kinds[kind] = kinds.get(kind, 0) + 1
                n += 1
                continue
            if kind in ("lba_small", "lba_batch", "lba_map"):
                if kind == "lba_small":
                    ws = [lba_window(int(rng.integers(0, 40))) for _ in range(int(rng.integers(1, 6)))]
                elif kind == "lba_batch":
                    ws = [lba_window(int(rng.integers(0, 40))) for _ in range(int(rng.choice([24, 60, 200])))]
                else:
                    if ("m",) not in pool:
                        pool[("m",)] = synth.make_window(77, n_free=300, n_fixed=2, n_points=12000, stereo=True, track_len=(3, 25), max_iterations=3)
                    ws = [pool[("m",)]]
                mode = int(rng.choice([-1, 0, 1]))
                live.set_pack_mode(mode)
                got = live.solve(ws)
                with lba.LbaSolver(0) as fresh:
                    fresh.set_pack_mode(mode)
                    ref = fresh.solve(ws)
                fields = LBA_FIELDS
            else:
                if kind == "liba_one":
                    ws = [inertial_window(int(rng.integers(0, 12)))]
                elif kind == "liba_batch":
                    ws = [inertial_window(int(rng.integers(0, 12))) for _ in range(int(rng.choice([3, 20, 130])))]
                elif kind == "liba_dense_map":
                    ws = [inertial_window(0, n_opt=int(rng.choice([60, 100])))]
                else:
                    ws = [inertial_window(0, n_opt=int(rng.choice([150, 250, 400])))]
                got = live.solve_inertial(ws)
                with lba.LbaSolver(0) as fresh:
                    ref = fresh.solve_inertial(ws)
                fields = LIBA_FIELDS
            for i, (a, b) in enumerate(zip(got, ref)):
                err = same(a, b, fields)
                if err:
                    print(f"MISMATCH call {n} ({kind}, {len(ws)} windows), window {i}: {err}", flush=True)
                    return 1
            kinds[kind] = kinds.get(kind, 0) + 1
            n += 1
            if n % 10 == 0:
                print(f"{n} calls ok {kinds}", flush=True)
    print(f"soak ok: {n} calls in one context, each equal bit for bit to the same call in a fresh context: {kinds}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
