#!/usr/bin/env python3
"""One SHA-256 per solver call over every output array and result scalar: run it on two builds and compare the lines.

Every solver of the library runs once on small committed inputs -- the tests/golden/*.npz fixtures and the synthetic makers
the tests use -- each call in a fresh context, through the raw C-ABI calls of tests/test_gpu_reuse.py (sentinel-filled
outputs, so an entry a kernel skips shows as well).  OSH_ZERO_NEW_BUFFERS=1: new allocations start zeroed.  Taken together the
inputs include a rejected Levenberg-Marquardt trial, an iteration ended by the three-bad-iterations rule, a frame with fewer
than 10 edges and a Sim3 problem that returns early; the `covers` column says which call showed what (read off the outputs).
A rejected trial and the three-bad-iterations stop can be read off the traces of the BA solvers and the trial counts of the pose
graphs only: the pose-only and OptimizeSim3 results carry no trace, so the column does not say which branches those took.
Usage: python profiles/solver_digest.py [output file]        (one line per call: name, sha256, covers)"""
import ctypes as C
import dataclasses
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
os.environ["OSH_ZERO_NEW_BUFFERS"] = "1"

from orb_slam3_study_kr_amd import capi, synth  # noqa: E402
from orb_slam3_study_kr_amd import synth_inertial as si  # noqa: E402
from orb_slam3_study_kr_amd import synth_sim3 as ss  # noqa: E402
import helpers  # noqa: E402
import test_gpu_reuse as tr  # noqa: E402


def calls():
    lba_golden = [helpers.load_lba_fixture(n)[0] for n in ("lba_tiny_stereo", "lba_tiny_mono", "lba_tiny_reject_mono", "lba_tiny_reject_stereo",
                                                            "lba_tiny_mixed", "lba_tiny_fisheye", "lba_tiny_rig")]
    out = [tr.lba_call(f"golden {i}", [w]) for i, w in enumerate(lba_golden)]
    # low noise and many iterations: the solve converges and ends on the three-bad-iterations rule
    out.append(tr.lba_call("converging window, 20 iterations", [synth.make_window(7, n_free=5, n_fixed=2, n_points=300, stereo=True, max_iterations=20)]))
    out.append(tr.lba_call("batch of 3", [synth.make_window(3000 + k, n_free=[3, 8, 20][k], n_fixed=1 + k, n_points=[400, 900, 1500][k], stereo=k != 1,
                                                             track_len=(3, 10), max_iterations=4) for k in range(3)]))
    out.append(tr.lba_call("global BA, 80 keyframes", [synth.make_window(46, n_free=80, n_fixed=1, n_points=2000, stereo=True, track_len=(3, 10), max_iterations=4)]))
    out.append(tr.liba_call("golden liba_tiny", [helpers.load_liba_fixture("liba_tiny")[0]]))
    out.append(tr.liba_call("golden liba_tiny_rig", [helpers.load_liba_fixture("liba_tiny_rig")[0]]))
    out.append(tr.liba_call("one window (block group)", [si.make_inertial_window(12, n_opt=10, n_points=900)]))
    out.append(tr.liba_call("batch of 3", [si.make_inertial_window(11 + k, n_opt=[4, 10, 14][k], n_points=600) for k in range(3)]))
    m = si.make_inertial_window(905, n_opt=40, n_fixed=0, n_points=1600, large=True)
    out.append(tr.liba_call("map BA, 40 keyframes", [dataclasses.replace(m, lambda_init=1e-5, max_iterations=3, link_robust=np.ones_like(m.link_robust))]))
    out.append(tr.pose_call("golden pose_tiny", [helpers.load_pose_fixture("pose_tiny")[0]]))
    out.append(tr.pose_call("golden pose_tiny_mono", [helpers.load_pose_fixture("pose_tiny_mono")[0]]))
    out.append(tr.pose_call("8-edge frame, mono, fisheye, rig, 1500 points",
                            [synth.make_pose_frame(61, n_points=8, stereo=True, outlier_frac=0.0), synth.make_pose_frame(54, n_points=400, stereo=False),
                             synth.make_pose_frame(52, n_points=700, stereo=False, outlier_frac=0.15, fisheye=True), synth.make_pose_frame(53, n_points=600, rig=True),
                             synth.make_pose_frame(62, n_points=1500, mixed_mono_frac=0.3)]))
    for n in ("posei_tiny_frame", "posei_tiny_keyframe", "posei_tiny_rig"):
        out.append(tr.posei_call(f"golden {n}", [helpers.load_posei_fixture(n)[0]]))
    mk = si.make_posei_frame
    out.append(tr.posei_call("mode 0 frames", [mk(40, mode=0, n_points=400), mk(41, mode=0, n_points=300, rec_init=True), mk(47, mode=0, n_points=40, outlier_frac=0.5)]))
    out.append(tr.posei_call("mode 1 frames", [mk(43, mode=1, n_points=300), mk(45, mode=1, n_points=300, rig=True), mk(46, mode=1, n_points=1500)]))
    s3 = dict(round2=ss.pack(ss.make_case(2, 300, 0.2)), early=ss.pack(ss.make_case(77, 14, 0.6)), kb8=ss.pack(ss.make_case(41, 300, 0.2, n_no_i2=3, kb8=True)),
              fixed=ss.pack(ss.make_case(301, 300, 0.2, n_no_i2=1, fix_scale=True)))
    out.append(tr.sim3_call("round 2, early return, KannalaBrandt8, fixed scale", [s3["round2"], s3["early"], s3["kb8"], s3["fixed"]]))
    out.append(tr.sim3_lin_call("linearize, pinhole", s3["round2"]))
    out.append(tr.sim3_lin_call("linearize, KannalaBrandt8", s3["kb8"]))
    out.append(tr.pgo_call("Sim3 graph, 300 vertices", tr._pgo_graph(300)))
    out.append(tr.pgo_call("Sim3 graph, 50 vertices, stereo", tr._pgo_graph(50, mono=False)))
    out.append(tr.pgo4_call("4-DoF graph, 300 vertices", tr._pgo4_graph(300)))
    out.append(tr.pgo4_call("4-DoF graph, 50 vertices", tr._pgo4_graph(50)))
    return out


def three_bad(chi0, trace, trials):
    """Did the solve end on g2o's three-bad-iterations rule?  (replayed from the chi2 trace)"""
    n_bad, chi = 0, chi0
    for c, q in zip(trace, trials):
        if q == 10:
            return False
        n_bad = n_bad + 1 if (chi - c) * 1e3 < chi else 0
        chi = c
    return n_bad >= 3


def covers(call, out):
    seen = set()
    for key in out:
        p = key.split(".")[0]
        if key.endswith(".trials_trace"):
            n = int(out[f"{p}.n_trace"][0])
            if (out[key][:n] > 1).any():
                seen.add("rejected trial")
            if n == int(out[f"{p}.iterations"][0]) and three_bad(float(out[f"{p}.chi2_initial"][0]), out[f"{p}.chi2_trace"][:n], out[key][:n]):
                seen.add("three bad iterations")
        if call.kind == "pose" and key.endswith(".rounds") and int(out[key][0]) == 1:
            seen.add("frame with fewer than 10 edges")
        if call.kind == "sim3" and key.endswith(".round2") and int(out[key][0]) == 0:
            seen.add("Sim3 early return")
        if call.kind in ("pgo", "pgo4") and key == "r.trials" and int(out[key][0]) > int(out["r.iterations"][0]):
            seen.add("rejected trial")
    return sorted(seen)


def digest(out):
    h = hashlib.sha256()
    for key in sorted(out):
        a = np.ascontiguousarray(out[key])
        h.update(key.encode())
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    lib = capi.load_library()
    if lib.osh_device_count() < 1:
        print("solver_digest: no HIP device visible")
        return 1
    lines, all_seen = [], set()
    for call in calls():
        out = tr.fresh_run(lib, call)
        seen = covers(call, out)
        all_seen.update(seen)
        lines.append(f"{call.kind}: {call.desc} | {digest(out)} | {', '.join(seen)}")
        print(lines[-1], flush=True)
    need = {"rejected trial", "three bad iterations", "frame with fewer than 10 edges", "Sim3 early return"}
    lines.append(f"covered: {sorted(all_seen)}; missing: {sorted(need - all_seen)}")
    print(lines[-1])
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text("\n".join(lines) + "\n")
    return 0 if need <= all_seen else 2


if __name__ == "__main__":
    sys.exit(main())
