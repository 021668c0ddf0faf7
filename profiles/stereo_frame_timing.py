#!/usr/bin/env python3
"""A rectified stereo frame, raw images in, keypoints, descriptors, mvuRight and mvDepth out, on one 752 x 480 pair (8 levels at
1.2, nfeatures 1000 per side, the synthetic pair of synth_stereo_pair), all variants in ONE process, alternating call by call:
  (a)  the path through the class before Frame::ExtractAndMatchStereo: ExtractBatchRaw(bKeepPyramid = true), which downloads both
       bordered pyramids, then ComputeStereoMatches, which packs and uploads them again;
  (a') the same two steps through the C-ABI: osh_orb_extract_raw with the levels downloaded, the level-0 scaling (numpy), then
       osh_orb_stereo_match on the downloaded levels;
  (b)  osh_orb_extract_raw without the download, the level-0 scaling (numpy), then osh_orb_stereo_match_resident by the tokens: it
       isolates the pyramid download, staging and upload;
  (c)  Frame::ExtractAndMatchStereo;
  (c') osh_orb_extract_stereo through the C-ABI, and its five phase times (osh_orb_set_profiling on, which synchronises between
       the phases) from osh_orb_extract_stereo_get_times;
  the two descriptor searches (osh_orb_stereo_set_row_search): the kernel phase of osh_orb_stereo_match_resident and the whole of
       osh_orb_extract_stereo with k_stereo_hamming and with the row lists.
(a) and (c) are the wall times of the member calls alone, measured inside the test library; the others are timed around the C calls
with result arrays sized once, as a caller that keeps its buffers does.  Then batches of 8 and 64 pairs through osh_orb_extract_stereo.
Every timed call ends in the call's own stream synchronisation.  --warmup calls first, then --reps timed calls per variant, median
and spread (max - min) in ms.  The results of (a'), (b) and (c') are compared bit for bit before anything is timed.  --json writes
the rows.

Per-kernel times of the stereo tail come from a separate run:
  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/stereo_frame_timing.py --reps 50 --batches ""
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import stereo_frame_cases as sc  # noqa: E402
import stereo_numpy as sn  # noqa: E402
from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import host as hostpy  # noqa: E402
from orb_slam3_study_kr_amd import synth_stereo_pair as sp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    rows = []

    def row(what, ts, **kw):
        ms, spread = float(np.median(ts)), float(max(ts) - min(ts))
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<78} {ms:9.4f} ms  +- {spread:.4f}", flush=True)
        return ms, spread

    named = sp.named_pair("pair_752x480_L8")
    p = sc.pair("pair_752x480_L8")
    items = [p["left"], p["right"]]
    with orb.OrbMatcher(0) as m:
        caps = [r["n_out"] for r in m.extract_raw(items, [0, 0])]
        print("keypoints left, right:", caps, flush=True)

        # (a'): extract_raw with the levels down, then the stage on them
        pf, _pr, _maps, _pk, _po = orb.prepare_args(items, False)
        ef_a, er_a, _ka, eo_a = orb.extract_raw_args(items, caps, True)
        capi.check(lib.osh_orb_extract_raw(m.ctx, 2, pf, ef_a, er_a, None), "osh_orb_extract_raw", lib)
        ex_a = orb._extract_outputs(er_a, eo_a)
        fr = sc.stereo_frame(p, ex_a[0], ex_a[1], ex_a[0]["levels"], ex_a[1]["levels"])   # the same images every call: the same levels
        sf_a, sr_a, _ska, so_a = orb.stereo_args([fr], False)
        # (b): extract_raw without the download, then the stage on the resident levels
        ef_b, er_b, _kb, eo_b = orb.extract_raw_args(items, caps, False)
        sf_b, sr_b, keep_b, so_b = orb.stereo_resident_args([fr], [(0, 0)], False)
        # (c'): the fused call
        pfc, efc, cpc, erc, csc, _kc, eoc, soc = orb.extract_stereo_args([p], caps, False, False, True)
        scale = np.asarray(p["left"]["scale"], np.float32)

        def rescale(ex_outs, stereo_keep):
            """pt *= scale[level] of the write-back for both sides, into the arrays the stereo frame points at."""
            for side, key in ((0, "lxy"), (1, "rxy")):
                s = scale[ex_outs[side]["level"][:caps[side]]][:, None]
                np.multiply(ex_outs[side]["xy"][:caps[side]], s, out=stereo_keep[key])

        def run_a():
            capi.check(lib.osh_orb_extract_raw(m.ctx, 2, pf, ef_a, er_a, None), "osh_orb_extract_raw", lib)
            rescale(eo_a, _ska[0][0])
            capi.check(lib.osh_orb_stereo_match(m.ctx, 1, sf_a, sr_a), "osh_orb_stereo_match", lib)

        def run_b():
            capi.check(lib.osh_orb_extract_raw(m.ctx, 2, pf, ef_b, er_b, None), "osh_orb_extract_raw", lib)
            rescale(eo_b, keep_b[0])
            sf_b[0].left_token, sf_b[0].right_token = er_b[0].pyramid_token, er_b[1].pyramid_token
            capi.check(lib.osh_orb_stereo_match_resident(m.ctx, 1, sf_b, sr_b), "osh_orb_stereo_match_resident", lib)

        def run_c():
            capi.check(lib.osh_orb_extract_stereo(m.ctx, 1, pfc, efc, cpc, erc, csc), "osh_orb_extract_stereo", lib)

        # descriptors and octaves of (b)'s frame are those of (a')'s first call: the same images give the same keypoints
        run_a(); run_b(); run_c()
        for name, got in (("(b)", so_b[0]), ("(c')", soc[0])):
            sn.assert_same(got, so_a[0], keys=("u_right", "depth"), what=name)
        print("matched (depth > 0):", int((so_a[0]["depth"] > 0).sum()), "of", caps[0], flush=True)

        raw_items = (dict(image=named["left"]), dict(image=named["right"]))
        member = lambda chain: hostpy.frame_extract_and_match_stereo(*raw_items, named["bf"], named["b"], raw=True, chain=chain)["call_ms"]

        def wall(fn_):
            t0 = time.perf_counter()
            fn_()
            return (time.perf_counter() - t0) * 1e3

        variants = {"(a)  ExtractBatchRaw(bKeepPyramid) + ComputeStereoMatches, the class": lambda: member(True),
                    "(a') osh_orb_extract_raw with levels + osh_orb_stereo_match": lambda: wall(run_a),
                    "(b)  osh_orb_extract_raw + osh_orb_stereo_match_resident": lambda: wall(run_b),
                    "(c)  Frame::ExtractAndMatchStereo, the class": lambda: member(False),
                    "(c') osh_orb_extract_stereo": lambda: wall(run_c)}
        ts = {k: [] for k in variants}
        for rep in range(a.warmup + a.reps):
            for k, fn_ in variants.items():
                t = fn_()
                if rep >= a.warmup:
                    ts[k].append(t)
        res = {k: row(f"1 pair 752x480x8: {k}", v) for k, v in ts.items()}
        keys = list(variants)
        for slow, fast in ((keys[0], keys[3]), (keys[1], keys[4]), (keys[1], keys[2]), (keys[2], keys[4])):
            d, s = res[slow][0] - res[fast][0], res[slow][1] + res[fast][1]
            print(f"  {slow[:4].strip()} - {fast[:4].strip()} = {d:+.4f} ms; sum of the two spreads {s:.4f} ms: {'beyond' if d > s else 'within'} the spreads", flush=True)

        m.set_profiling(True)
        ph = []
        for k in range(a.warmup + a.reps):
            run_c()
            if k >= a.warmup:
                ph.append(m.extract_stereo_times())
        m.set_profiling(False)
        ph = np.array(ph)
        for k, phase in enumerate(("checks, preparation, pyramid", "detector", "quadtree", "orientation, descriptors, download, write-back", "stereo tail")):
            row(f"1 pair 752x480x8:   (c') {phase}", ph[:, k])

        # the two descriptor searches of the entries on resident pyramids, alternating: the kernel phase of the resident stage
        # (synchronised on both sides; the search, the SAD window and the median cut) and the fused call as a whole
        run_c()

        def stage_kernels():
            sf_b[0].left_token, sf_b[0].right_token = erc[0].pyramid_token, erc[1].pyramid_token   # the pair the fused call left resident
            capi.check(lib.osh_orb_stereo_match_resident(m.ctx, 1, sf_b, sr_b), "osh_orb_stereo_match_resident", lib)
            return float(m.stereo_times()[2])

        searches = {"k_stereo_hamming": False, "row lists": True}
        kt, ct = {k: [] for k in searches}, {k: [] for k in searches}
        for rep in range(a.warmup + a.reps):
            for k, enable in searches.items():
                m.set_stereo_row_search(enable)
                m.set_profiling(True)
                t = stage_kernels()
                m.set_profiling(False)
                w = wall(run_c)
                if rep >= a.warmup:
                    kt[k].append(t); ct[k].append(w)
        m.set_stereo_row_search(True)
        sres = {k: row(f"1 pair 752x480x8: kernels of the resident stage, search = {k}", v) for k, v in kt.items()}
        for k, v in ct.items():
            row(f"1 pair 752x480x8: (c') osh_orb_extract_stereo, search = {k}", v)
        d, s = sres["k_stereo_hamming"][0] - sres["row lists"][0], sres["k_stereo_hamming"][1] + sres["row lists"][1]
        print(f"  k_stereo_hamming - row lists = {d:+.4f} ms; sum of the two spreads {s:.4f} ms: {'beyond' if d > s else 'within'} the spreads", flush=True)

        pairs4 = []
        for k in range(4):
            left, right = sp.make_pair(31 + k, 480, 752)
            pairs4.append(sc.custom_pair(left, right, 8, 1000, bf=named["bf"], b=named["b"]))
        for batch in (int(b) for b in a.batches.split(",") if b):
            pairs = [pairs4[k % 4] for k in range(batch)]
            sized = m.extract_stereo(pairs, [0] * (2 * batch), raw=True)
            bcaps = [r[side]["n_out"] for r in sized for side in ("left", "right")]
            bpf, bef, bcp, ber, bcs, _bk, _beo, _bso = orb.extract_stereo_args(pairs, bcaps, False, False, True)

            def run_batch():
                capi.check(lib.osh_orb_extract_stereo(m.ctx, batch, bpf, bef, bcp, ber, bcs), "osh_orb_extract_stereo", lib)

            reps = a.reps if batch <= 8 else max(a.reps // 5, 10)
            bt = [wall(run_batch) for _ in range(a.warmup + reps)][a.warmup:]
            ms, _ = row(f"{batch} pairs 752x480x8: osh_orb_extract_stereo ({sum(bcaps)} keypoints)", bt, pairs_per_s=batch * 1e3 / float(np.median(bt)))
            print(f"  {ms / batch:.4f} ms per pair", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
