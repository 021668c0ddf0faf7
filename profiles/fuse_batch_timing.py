#!/usr/bin/env python3
"""Fuse batch timing: osh_orb_fuse_search (the search of ORBmatcher::Fuse for one map point list and K target keyframes in one
call) on (a) 1 x 1000 points x 1500 keypoints, (b) 20 targets (the stereo SearchInNeighbors shape), (c) 40 targets (mono with
second neighbours), (d) 30 targets x 5000 points in Sim3 mode with th = 4 (SearchAndFuse) -- against two baselines on the same data:

  loop   what the loop of single Fuse calls does on the device today, target by target: osh_orb_upload of the target's descriptors,
         the surviving points' descriptors and their candidate lists, osh_orb_match, osh_orb_download (K uploads, K launches, K
         downloads).  The lists are built beforehand, so the host projection and list building that ORBmatcher::Fuse also pays per
         call (csrc/host/ORBmatcher.cc, fuse_search) is NOT in this figure: it is a lower bound of the loop.
  cpu    osh_host_fuse_search_cpu: the statements of csrc/orb_fuse.h compiled for the host at the library's optimisation level, one
         thread, everything included (binning, projection, search).

The batch is timed by wall clock unprofiled (the call ends in its own stream synchronisation) and split into staging, upload,
kernels and download by its phase clock (osh_orb_set_profiling on, which synchronises between the phases).  --warmup calls first,
then --reps timed calls, median and spread (max - min) in ms.  Argument and result arrays are built once.  Before anything is
timed the batch is compared with the host build in every bit of every output, and the loop's best index and distance with the
batch's for every searched pair.  --json writes the rows."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from orb_slam3_study_kr_amd import capi, orb  # noqa: E402
from orb_slam3_study_kr_amd import synth_fuse as sf  # noqa: E402

fn = sf   # the mode and stage constants, NAMES and same_bits

F = np.float32
SHAPES = {"a": (1, 1000, 1500, fn.CHI2, 3.0), "b": (20, 1000, 1500, fn.CHI2, 3.0), "c": (40, 1000, 1500, fn.CHI2, 3.0),
          "d": (30, 5000, 1500, fn.SIM3, 4.0)}


def timed(fn_, reps, warmup):
    for _ in range(warmup):
        fn_()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn_()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def candidate_lists(t, pts, out_k, mode):
    """The explicit lists ORBmatcher::Fuse uploads for one target today: per surviving point (stage SEARCHED) the keypoints of
    GetFeaturesInArea in its order that pass the level and chi2 gates.  Vectorised float32, the same single operations."""
    _, inv_sigma2, _ = t.level_tables()
    gx, gy, winv, hinv = F(t.grid_min[0]), F(t.grid_min[1]), F(t.cell_inv[0]), F(t.cell_inv[1])

    def c_round(v):
        v = v.astype(np.float64)
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)
    px, py = c_round((t.key_xy[:, 0] - gx) * winv), c_round((t.key_xy[:, 1] - gy) * hinv)
    in_grid = (px >= 0) & (px < t.cols) & (py >= 0) & (py < t.rows)
    order = np.lexsort((np.arange(t.n_keys), py, px))          # cell-major (ix, then iy), keypoint order inside a cell
    order = order[in_grid[order]]
    q = np.flatnonzero(out_k["stage"] == fn.SEARCHED)
    u, v, ur, r, lev = (out_k[n][q][:, None] for n in ("u", "v", "ur", "radius", "level"))
    kx, ky, ko = t.key_xy[order, 0][None, :], t.key_xy[order, 1][None, :], t.key_octave[order][None, :]
    ok = (np.abs(kx - u) < r) & (np.abs(ky - v) < r) & (ko >= lev - 1) & (ko <= lev)
    if mode == fn.CHI2:
        ex, ey = u - kx, v - ky
        e2 = ex * ex + ey * ey
        inv = inv_sigma2[t.key_octave[order]][None, :]
        mono = (e2 * inv).astype(np.float64) <= 5.99
        if t.key_uright is not None:
            kur = t.key_uright[order][None, :]
            er = ur - kur
            stereo = ((e2 + er * er) * inv).astype(np.float64) <= 7.8
            ok &= np.where(kur >= 0, stereo, mono)
        else:
            ok &= mono
    off = np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int32)
    idx = np.broadcast_to(order[None, :], ok.shape)[ok].astype(np.int32)
    return q, off, idx


def loop_call(t, pts, q, off, idx):
    """The osh_orb_batch of one target's search as the loop uploads it, and its result arrays."""
    a = dict(q=np.ascontiguousarray(pts.desc[q]), t=np.ascontiguousarray(t.desc), off=off, idx=idx if idx.size else np.zeros(1, np.int32),
             base=np.zeros(1, np.int64))
    b = capi.OrbBatch()
    b.n_pairs, b.n_query, b.n_train = 1, int(q.size), t.n_keys
    b.query_desc, b.train_desc = capi.ptr(a["q"], capi.c_uint8_p), capi.ptr(a["t"], capi.c_uint8_p)
    b.train_level = C.cast(None, capi.c_int32_p)
    b.cand_off, b.cand_idx, b.pair_cand_base = capi.ptr(a["off"], capi.c_int32_p), capi.ptr(a["idx"], capi.c_int32_p), capi.ptr(a["base"], capi.c_int64_p)
    outs = [np.zeros(max(int(q.size), 1), np.int32) for _ in range(6)]
    return b, a, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=10)
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, host = capi.load_library(), capi.load_host_library()
    if lib.osh_device_count() < 1:
        raise SystemExit("fuse_batch_timing: no HIP device visible")
    rows = []

    def row(what, ms, spread, **kw):
        rows.append(dict(what=what, ms=ms, spread_ms=spread, **kw))
        print(f"{what:<66} {ms:9.4f} ms  +- {spread:.4f}", flush=True)

    with orb.OrbMatcher(0) as m, orb.OrbMatcher(0) as single:
        for shape in a.shapes.split(","):
            K, P, N, mode, th = SHAPES[shape]
            targets, pts = sf.make_case(900 + ord(shape), K, P, N, stereo=(shape in "bd"), th=th)
            name = f"({shape}) {K} x {P} points x {N} keys"
            ct, cp, cr, _keep, out = orb.fuse_args(targets, pts)
            ht, hp, hr, _hkeep, hout = orb.fuse_args(targets, pts)

            def device():
                capi.check(lib.osh_orb_fuse_search(m.ctx, K, ct, C.byref(cp), mode, C.byref(cr)), "osh_orb_fuse_search", lib)

            def cpu():
                if host.osh_host_fuse_search_cpu(K, ht, C.byref(hp), mode, C.byref(hr), None) != 0:
                    raise RuntimeError("osh_host_fuse_search_cpu")
            device(); cpu()
            assert fn.same_bits(out, hout) == [], name
            calls = []
            for k, t in enumerate(targets):
                q, off, idx = candidate_lists(t, pts, {n: hout[n][k] for n in fn.NAMES}, mode)
                calls.append((q, k) + loop_call(t, pts, q, off, idx))

            def loop():
                for q, _k, b, _a, outs in calls:
                    if q.size == 0:
                        continue
                    capi.check(lib.osh_orb_upload(single.ctx, C.byref(b)), "osh_orb_upload", lib)
                    capi.check(lib.osh_orb_match(single.ctx), "osh_orb_match", lib)
                    capi.check(lib.osh_orb_download(single.ctx, *[capi.ptr(o, capi.c_int32_p) for o in outs]), "osh_orb_download", lib)
            loop()
            # the last target's outputs are still in place; check every target once, outside the timing
            for q, k, b, _a, outs in calls:
                if q.size == 0:
                    continue
                capi.check(lib.osh_orb_upload(single.ctx, C.byref(b)), "osh_orb_upload", lib)
                capi.check(lib.osh_orb_match(single.ctx), "osh_orb_match", lib)
                capi.check(lib.osh_orb_download(single.ctx, *[capi.ptr(o, capi.c_int32_p) for o in outs]), "osh_orb_download", lib)
                assert np.array_equal(outs[0][:q.size], out["best_idx"][k][q]) and np.array_equal(outs[1][:q.size], out["best_dist"][k][q]), (name, k)
            searched = int((out["stage"] >= fn.EMPTY).sum())
            found = int((out["best_idx"] >= 0).sum())
            ms, sp = timed(device, a.reps, a.warmup)
            row(f"{name}: osh_orb_fuse_search (wall)", ms, sp, pairs=K * P, pairs_past_the_gates=searched, pairs_with_a_best=found)
            m.set_profiling(True)
            phases = []
            for k in range(a.warmup + a.reps):
                device()
                if k >= a.warmup:
                    phases.append(m.fuse_times())
            m.set_profiling(False)
            ph = np.array(phases)
            for k, phase in enumerate(("staging", "upload", "kernels", "download")):
                row(f"{name}:   {phase}", float(np.median(ph[:, k])), float(ph[:, k].max() - ph[:, k].min()))
            lms, lsp = timed(loop, a.reps, a.warmup)
            row(f"{name}: loop of {K} single searches, lists prebuilt (wall)", lms, lsp, device_calls=3 * sum(1 for c in calls if c[0].size))
            cms, csp = timed(cpu, a.cpu_reps, 2)
            row(f"{name}: CPU, one thread (wall)", cms, csp)
            print(f"  ({K * P} pairs, {searched} past the gates, {found} with a best; batch / loop = {ms / lms:.3f}, batch / CPU = {ms / cms:.3f})", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
