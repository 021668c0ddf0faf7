"""Named frames and probes of the stage tests of k_pose_opt (tests/test_pose_stage_cpu.py, tests/test_gpu_pose_stages.py), all built by code
from synth.make_pose_frame, and their references, computed once per process:

    frame(name)       a synth.PoseFrame with the default budgets (10,10,10,10) and thresholds (5.991 / 7.815)
    probe(name)       a frame with budgets / thresholds of its own, "<frame>/<probe>":
                        r<k>  budgets (k,0,0,0), thresholds BIG: k robust iterations, seen through chi2_final[0], iterations[0], edge_chi2
                        n<k>  budgets (0,0,0,k), thresholds BIG: k non-robust iterations, pose_qt exported too
                        full  the frame as it is
                        further ones are listed under PROBE_BUILDERS
    refs(name)        namespace(ld, f64, oracle): pose_stage_numpy in long double and float64, oracle/pose_oracle.c

The kernel's budgets and thresholds are inputs, so a probe shows one stage of the kernel through its ordinary outputs.  Every probe is
built so that nothing compared depends on an edge's chi2 before its first evaluation (the reference library leaves that undefined).
"""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

import pose_stage_numpy as ps
from orb_slam3_study_kr_amd import synth

BIG = ps.BIG
EPS = 2.0 ** -52

# M of the bound d_dev <= max(M d64, floor): the smallest power of two >= 4 x the worst d_dev / d64 measured on an MI355X (6.54, see the
# table in test_gpu_pose_stages.py); the 4 is headroom for a compiler release that contracts other products
M = 32
FLOOR = 8 * EPS                                   # 8 ulp of the quantity (every distance below is relative to its quantity)
CAPS = dict(chi2_final=1e-10, trans=1e-10, rot=1e-10, edge_chi2=1e-9)

SEAM_SIZES = (9, 10, 255, 256, 257, 1023, 1024, 1025, 1281, 2809)
# the far frames in which Levenberg-Marquardt rejects trials: (seed, pose_noise, stereo) and, for the robust (0) and the non-robust (3)
# round, the iteration (from 0) whose long-double trace must show qmax > 1
REJECT = {
    "reject-89": (89, (0.8, 3.0), False, {0: 0, 3: 0}),
    "reject-88": (88, (1.5, 3.0), False, {0: 4, 3: 0}),
    "reject-78": (78, (0.8, 3.0), False, {0: 2, 3: 2}),
    "reject-88s": (88, (1.5, 3.0), True, {3: 5}),
}
ONE_ITERATION_FRAMES = tuple(f"seam-{n}" for n in SEAM_SIZES) + ("mono", "kb8", "rig", "rig-1100", "neg-w")
TRAJECTORY_FRAMES = ("seam-257", "seam-1025", "mono", "kb8") + tuple(REJECT)


def cut(f, index):
    """The frame with the edges `index` only (in that order)."""
    index = np.asarray(index, dtype=np.int64)
    return dataclasses.replace(f, points=f.points[index], edge_kind=f.edge_kind[index], edge_obs=f.edge_obs[index],
                               edge_info=f.edge_info[index], outlier_mask=None).normalise()


def with_probe(f, budgets=(10, 10, 10, 10), mono=(BIG,) * 4, stereo=(BIG,) * 4):
    return dataclasses.replace(f, iterations=tuple(budgets), chi2_mono=tuple(mono), chi2_stereo=tuple(stereo))


def exact_frame():
    """Twelve pinhole points whose residuals are exactly zero in every arithmetic: identity pose, z = fx fy / 4096, x = jx fy / 4096,
    y = jy fx / 4096 with integers jx, jy of at most five significant bits, so that fx x, fy y and both quotients by z are exact.
    b = 0, the step is zero, the trial's chi2 equals the current one: the first iteration of every round ends on rho == 0."""
    base = synth.make_pose_frame(21, n_points=20, stereo=False, mixed_mono_frac=0.0)
    fx, fy, cx, cy = (float(v) for v in base.cam[:4])
    j = np.array([[-192, -96], [-128, 80], [-64, -32], [-8, 120], [0, 0], [16, -144], [40, 72], [96, 8], [136, -60], [176, 144],
                  [-30, 30], [76, -72]], dtype=np.float64)
    z = fx * fy / 4096
    X = np.stack([j[:, 0] * fy / 4096, j[:, 1] * fx / 4096, np.full(12, z)], axis=1)
    obs = np.stack([j[:, 0] + cx, j[:, 1] + cy, np.full(12, -1.0)], axis=1)
    assert np.all(fx * X[:, 0] / z == j[:, 0]) and np.all(fy * X[:, 1] / z == j[:, 1])
    return dataclasses.replace(base, pose_qt=np.array([0, 0, 0, 1.0, 0, 0, 0]), points=X, edge_obs=obs, edge_kind=np.zeros(12, np.uint8),
                               edge_info=np.ones(12), outlier_mask=None, gt_pose_qt=None).normalise()


@functools.lru_cache(maxsize=None)
def _seam():
    f = synth.make_pose_frame(27, n_points=3000)
    assert f.n_edges == 2809
    return f


@functools.lru_cache(maxsize=None)
def frame(name):
    if name == "seam-1281-rotated":                     # the last 200 edges first: cached and global-memory edges trade places
        return cut(_seam(), rotation_1281())
    if name.startswith("seam-"):
        return cut(_seam(), np.arange(int(name[5:])))
    if name == "mono":
        return cut(synth.make_pose_frame(24, stereo=False, mixed_mono_frac=0.0), np.arange(300))
    if name == "kb8":
        return cut(synth.make_pose_frame(28, stereo=False, fisheye=True), np.arange(300))
    if name == "rig":
        return cut(synth.make_pose_frame(33, rig=True, n_points=900), np.arange(300))
    if name == "rig-1100":                              # body and KannalaBrandt8 edges beyond the 1024 cached ones (the generator gives 2949)
        return cut(synth.make_pose_frame(33, rig=True, n_points=3000), np.arange(1100))
    if name in REJECT:
        seed, noise, stereo, _ = REJECT[name]
        return synth.make_pose_frame(seed, n_points=40, pose_noise=noise, outlier_frac=0.3, stereo=stereo)
    if name == "zero-info":
        f = frame("seam-257")
        return dataclasses.replace(f, edge_info=np.zeros_like(f.edge_info))
    if name == "neg-w":                                 # setEstimate normalises: q and -1.7 q are the same rotation
        f = frame("seam-257")
        q = f.pose_qt.copy()
        q[:4] *= -1.7
        return dataclasses.replace(f, pose_qt=q)
    if name == "exact":
        return exact_frame()
    if name == "empty":
        return cut(_seam(), np.arange(0))
    raise KeyError(name)


def rotation_1281():
    return np.concatenate([np.arange(1081, 1281), np.arange(1081)])


# ------------------------------------------------------------------------------------------------------------- probes
def _median_after_round0(fname):
    """The median edge chi2 at the classification of round 0 (long double), moved off every edge's value."""
    c = np.sort(refs(f"{fname}/full-big").ld.round_chi2[0].astype(np.float64))
    return float(np.float32(0.5 * (c[len(c) // 2 - 1] + c[len(c) // 2])))


def strict_edge(fname, kind):
    """An edge of `kind` whose round-3 chi2 is at least 2^-30 (relative) from every float32 rounding midpoint and at least 1e-6 from
    every other edge's: returns (edge, float32 threshold equal to its rounded chi2)."""
    r = refs(f"{fname}/full-big").ld
    c = r.round_chi2[3]
    f = frame(fname)
    order = np.argsort(c.astype(np.float64))
    for e in order[len(order) // 3:]:
        if f.edge_kind[e] != kind:
            continue
        th = np.float32(c[e])
        lo, hi = np.nextafter(th, np.float32(-np.inf)), np.nextafter(th, np.float32(np.inf))
        mids = (np.longdouble(lo) + np.longdouble(th)) / 2, (np.longdouble(hi) + np.longdouble(th)) / 2
        if min(abs(c[e] - m) for m in mids) < 2.0 ** -30 * c[e]:
            continue
        others = np.delete(c, e)
        if np.abs(others - c[e]).min() < 1e-6 * c[e]:
            continue
        return int(e), th
    raise AssertionError("no edge qualifies")


def _strict(fname, kind, below):
    e, th = strict_edge(fname, kind)
    if below:
        th = np.nextafter(th, np.float32(-np.inf))
    th4 = (BIG, BIG, BIG, float(th))
    return with_probe(frame(fname), mono=th4 if kind == ps.MONO else (BIG,) * 4, stereo=th4 if kind == ps.STEREO else (BIG,) * 4)


def _readmit(fname, budgets, rounds):
    t = _median_after_round0(fname)
    th = tuple(t if r in rounds else BIG for r in range(4))
    return with_probe(frame(fname), budgets, th, th)


PROBE_BUILDERS = {
    "full": lambda fn: frame(fn),
    "full-big": lambda fn: with_probe(frame(fn)),                                          # four rounds, nothing classified out
    # (t, BIG, BIG, BIG), t the median chi2 after round 0: half the edges sit out round 1 and are re-admitted after it
    "readmit": lambda fn: _readmit(fn, (10, 10, 10, 10), (0,)),
    "readmit-stop2": lambda fn: _readmit(fn, (10, 10, 0, 0), (0,)),                        # edge_chi2 as round 1 leaves it
    "readmit-all4": lambda fn: _readmit(fn, (10, 10, 10, 10), (0, 1, 2, 3)),               # a non-trivial final outlier set
    "allout": lambda fn: with_probe(frame(fn), (10, 10, 10, 10), (-1.0, BIG, BIG, BIG), (-1.0, BIG, BIG, BIG)),
    "allout-stop2": lambda fn: with_probe(frame(fn), (10, 10, 0, 0), (-1.0, BIG, BIG, BIG), (-1.0, BIG, BIG, BIG)),
    "strict-mono-at": lambda fn: _strict(fn, ps.MONO, False),
    "strict-mono-below": lambda fn: _strict(fn, ps.MONO, True),
    "strict-stereo-at": lambda fn: _strict(fn, ps.STEREO, False),
    "strict-stereo-below": lambda fn: _strict(fn, ps.STEREO, True),
}


@functools.lru_cache(maxsize=None)
def probe(name):
    fname, kind = name.rsplit("/", 1)
    if kind in PROBE_BUILDERS:
        return PROBE_BUILDERS[kind](fname)
    k = int(kind[1:])
    assert kind[0] in "rn"
    return with_probe(frame(fname), (k, 0, 0, 0) if kind[0] == "r" else (0, 0, 0, k))


def oracle_run(f):
    from oracle import binding
    return binding.pose_optimize(f)


@functools.lru_cache(maxsize=None)
def refs(name):
    ps.require_extended()
    f = probe(name)
    return SimpleNamespace(ld=ps.optimize(f, np.longdouble), f64=ps.optimize(f, np.float64), oracle=oracle_run(f))


def trajectory_length(fname, mode):
    """K: the first budget that the long-double reference does not use up (10 when it uses every one)."""
    rnd = 0 if mode == "r" else 3
    return min(int(refs(f"{fname}/{mode}10").ld.iterations[rnd]) + 1, 10)


def trajectory_probes():
    return [f"{fn}/{mode}{k}" for fn in TRAJECTORY_FRAMES for mode in "rn" for k in range(1, trajectory_length(fn, mode) + 1)]


def settled(name):
    """A trajectory probe's stop decision is settled when long double, float64 and the oracle report the same iteration counts."""
    r = refs(name)
    return np.array_equal(r.ld.iterations, r.f64.iterations) and np.array_equal(r.ld.iterations, r.oracle.iterations)


ONE_ITERATION_PROBES = [f"{fn}/{m}1" for fn in ONE_ITERATION_FRAMES for m in "rn"]
STORAGE_PROBES = [f"{fn}/{p}" for fn in ("seam-1281", "seam-1281-rotated", "seam-257") for p in ("r3", "n3")]
CLASSIFICATION_PROBES = [f"seam-257/{p}" for p in PROBE_BUILDERS if p not in ("full", "full-big")] + ["rig/readmit", "rig/allout"]
STOP_PROBES = ["zero-info/full", "exact/full", "seam-9/full-big"]


def all_probes():
    return ONE_ITERATION_PROBES + trajectory_probes() + STORAGE_PROBES + CLASSIFICATION_PROBES + STOP_PROBES


# ------------------------------------------------------------------------------------------------------------- distances
def distances(got, ld, pose=True):
    """Distance of a result (device, oracle or float64 reference) from the long-double reference, each relative to its quantity:
    chi2_final (per round, relative), edge_chi2 (relative to max(chi2, 1e-3), over the edges that were evaluated), trans (relative
    translation), rot (rad).  Differences are formed in long double."""
    L = np.longdouble
    d = {}
    g, r = np.asarray(got.chi2_final).astype(L), ld.chi2_final
    d["chi2_final"] = float(np.max(np.abs(g - r) / np.where(r != 0, np.abs(r), L(1))))
    ev = ld.evaluated
    if ev.any():
        g, r = np.asarray(got.edge_chi2).astype(L)[ev], ld.edge_chi2[ev]
        d["edge_chi2"] = float(np.max(np.abs(g - r) / np.maximum(r, L(1e-3))))
    if pose:
        g, r = np.asarray(got.pose_qt).astype(L), ld.pose_qt
        d["trans"] = float(np.sqrt(((g[4:] - r[4:]) ** 2).sum()) / max(np.sqrt((r[4:] ** 2).sum()), L(1e-12)))
        gq = g[:4] / np.sqrt((g[:4] ** 2).sum())
        rel = ps.quat_mul(gq, np.concatenate([-r[:3], r[3:4]]))
        d["rot"] = float(2 * np.arctan2(np.sqrt((rel[:3] ** 2).sum()), np.abs(rel[3])))
    return d


def bounds(name):
    """Per quantity: (d64, bound) with d64 the oracle's distance from the long-double reference and bound = max(M d64, FLOOR)."""
    r = refs(name)
    d64 = distances(r.oracle, r.ld)
    return {k: (v, max(M * v, FLOOR)) for k, v in d64.items()}
