"""Named cases and probes of the stage tests of k_sim3_opt (tests/test_sim3_stage_cpu.py, tests/test_gpu_sim3_stages.py), built by code
directly as packs (the dicts synth_sim3.problem() takes), and their references, computed once per process:

    case(name)        a pack with the budgets (5, 10, 5) and th2 = 10
    probe(name)       a pack with budgets / th2 of its own, "<case>/<probe>":
                        e     budgets (0,0,0): both edges' chi2 at the input S12 and the final classification (n >= 10)
                        r<k>  budgets (k,0,0): k robust iterations; iterations[0], chi2_end[0], outlier1, n_bad, and, when at least 10
                              inliers remain, S12 after round 1 and every pair's chi2 there (the outliers' when the last trial was taken)
                        n<k>  budgets (0,k,k): k plain iterations over every pair, S12 and the final classification
                        full  (5,10,5);  b532  (5,3,2)
                        further ones are listed under PROBE_BUILDERS
    refs(name)        namespace(ld, f64): sim3_stage_numpy.run in long double and in float64
    lin_refs(case, robust)   the same for osh_sim3_linearize (robust: th2 of the case; plain: th2 = 1e30f)

Distances, caps and the bound d_dev <= max(M d64, 8 ulp) are at the end.
"""
import functools
from types import SimpleNamespace

import numpy as np

import pgo_numpy as pn
import sim3_stage_numpy as s3

F32 = np.float32
EPS = 2.0 ** -52
FLOOR = 8 * EPS
# M of the bound d_dev <= max(M d64, FLOOR): the smallest power of two >= 4 x the worst d_dev / d64 measured on an MI355X (3.29, see the table
# in test_gpu_sim3_stages.py); the 4 is headroom for a compiler release that orders the sums or contracts differently
M = 16
# CAP_INPUT: chi2 at a given S12 (a pair's relative to max(chi2, 1e-3), and the sums), the project's cap for such quantities.
# CAP_DIFF: everything that passes through the 1e-9 central differences (scaled H and b, S12 after iterations, chi2_end): the float64
# forward error of (e+ - e-) / 2e-9, about 1e-3 absolute for projections up to 1e3 px against Jacobian columns of at least 1e2.
# A pair's chi2 at an estimate that is not exported (trial_chi2: the last trial of round 1 where round 2 moved on or did not run) passes
# through the differences too and has CAP_DIFF.  It moves with that estimate, d chi2 = 2 sqrt(info chi2) sqrt(info) |J dS|, so its error
# is proportional to sqrt(chi2), not to chi2: it is taken relative to max(chi2, 1), one sigma, where it is at most 2 |J dS| px whatever
# the pair's residual (relative to max(chi2, 1e-3) a pair of 0.03 px would weigh thirty times a pair at the threshold)
CAP_INPUT, CAP_DIFF = 1e-10, 1e-5
CAPS = dict(pair_chi2=CAP_INPUT, trial_chi2=CAP_DIFF, chi2_end=CAP_DIFF, rot=CAP_DIFF, trans=CAP_DIFF, scale=CAP_DIFF)
LIN_CAPS = dict(H=CAP_DIFF, b=CAP_DIFF, chi2=CAP_INPUT)

PINHOLE = np.array([458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0])
PINHOLE_B = np.array([535.4, 539.2, 320.1, 247.6, 0, 0, 0, 0])
KB8 = np.array([190.978, 190.973, 254.932, 256.897, 0.00348238, 0.000715034, -0.00205323, 0.000202937])
KB8_B = np.array([190.442, 190.434, 252.597, 254.917, 0.00340031, 0.00176627, -0.00266312, 0.000329964])
TH2 = 10.0

SEAM_SEED = 32
SEAM_SIZES = (1, 9, 10, 63, 64, 65, 255, 256, 257, 513)
CAMS = ("pp", "kk", "pk", "kp")
SCALES = (0.5, 1.0, 3.0)


def _quat(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([w / th * np.sin(th / 2), [np.cos(th / 2)]])


def _project(cam, kb8, X):
    return s3.project(cam, kb8, np.asarray(X, np.float64))[0]


def make_pack(seed, n, cams="pp", scale=None, fix_scale=False, n_norm=0, outlier_frac=0.2, gross=0, noise_px=0.7, perturb=1.0):
    """n pairs seen by camera 1 (`cams[0]`: p Pinhole, k KannalaBrandt8) and camera 2 (`cams[1]`) through a known S12 of the given scale
    (x1 = S12 x2): points and keypoints rounded to float32 as the host's walk leaves them, pixel noise, a fraction of moderate outliers
    (2 - 12 px off, on both sides of the Huber threshold), `gross` pairs 60 px off, `n_norm` pairs whose obs2 are normalised coordinates
    with the information of level 0 (the i2 < 0 pairs), and an initial estimate `perturb` times as far off as Sim3Solver leaves it."""
    rng = np.random.default_rng(seed)
    kb1, kb2 = cams[0] == "k", cams[1] == "k"
    cam1 = KB8 if kb1 else PINHOLE
    cam2 = KB8_B if kb2 else PINHOLE_B
    if scale is None:
        scale = 1.0 if fix_scale else float(rng.uniform(0.7, 1.4))
    q12 = _quat(rng.normal(size=3) * 0.08)
    S_true = np.concatenate([q12, rng.normal(size=3) * 0.15, [scale]])
    dq = _quat(rng.normal(size=3) * 0.004 * perturb)
    S12 = np.concatenate([pn.quat_mul(dq, q12), S_true[4:7] + rng.normal(size=3) * 0.01 * perturb,
                          [scale if fix_scale else scale * (1 + 0.01 * perturb * rng.normal())]])
    S12[:4] /= np.linalg.norm(S12[:4])
    if kb1 or kb2:
        d = rng.normal(size=(n, 3)); d[:, 2] = np.abs(d[:, 2]) + 0.9
    else:
        d = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.45, 0.45, n), np.ones(n)], -1)
    X1 = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 8.0, (n, 1))
    X2 = pn.sim3_map(pn.sim3_inverse(S_true), X1)
    assert np.all(X1[:, 2] > 0.3) and np.all(X2[:, 2] > 0.3 / max(scale, 1.0))
    obs1 = _project(cam1, kb1, X1) + rng.normal(size=(n, 2)) * noise_px
    obs2 = _project(cam2, kb2, X2) + rng.normal(size=(n, 2)) * noise_px
    levels = (1.0 / 1.2 ** (2 * np.arange(8))).astype(F32).astype(np.float64)
    info1, info2 = levels[rng.integers(0, 8, n)], levels[rng.integers(0, 8, n)]
    n_out = int(round(outlier_frac * n))
    if n_out:
        sel = rng.choice(n, n_out, replace=False)
        ang = rng.uniform(0, 2 * np.pi, n_out)
        off = rng.uniform(2.0, 12.0, n_out)[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
        half = rng.random(n_out) < 0.5
        obs1[sel[half]] += off[half]
        obs2[sel[~half]] += off[~half]
    if gross:
        sel = rng.choice(n, gross, replace=False)
        obs1[sel] += 60.0
    X1, X2 = X1.astype(F32).astype(np.float64), X2.astype(F32).astype(np.float64)
    obs1, obs2 = obs1.astype(F32).astype(np.float64), obs2.astype(F32).astype(np.float64)
    if n_norm:
        sel = rng.choice(n, n_norm, replace=False)
        invz = F32(1) / X2[sel, 2].astype(F32)
        obs2[sel] = np.stack([X2[sel, 0].astype(F32) * invz, X2[sel, 1].astype(F32) * invz], -1).astype(np.float64)
        info2[sel] = levels[0]
    norm = np.zeros(n, bool)
    if n_norm:
        norm[sel] = True
    return dict(index=np.arange(n, dtype=np.int32), X1c=X1, X2c=X2, obs1=obs1, obs2=obs2, info1=info1, info2=info2,
                cam1=cam1.copy(), cam2=cam2.copy(), kb8_1=int(kb1), kb8_2=int(kb2), S12=S12, fix_scale=bool(fix_scale),
                th2=float(F32(TH2)), iterations=s3.BUDGETS, normalised=norm)


PAIR_ARRAYS = ("X1c", "X2c", "obs1", "obs2", "info1", "info2", "normalised")


def cut(pk, index):
    """The pack with the pairs `index` only (in that order)."""
    index = np.asarray(index, dtype=np.int64)
    out = dict(pk)
    for k in PAIR_ARRAYS:
        out[k] = pk[k][index]
    out["index"] = np.arange(len(index), dtype=np.int32)
    return out


def rotation_100(n):
    return np.concatenate([np.arange(100, n), np.arange(100)])


# seeds found with the float64 reference on the CPU for what the names say; test_sim3_stage_cpu.py asserts that they still do
REJECT = ("reject-110", 100.0)          # a start 100 times as far off whose first plain trial Levenberg-Marquardt rejects
LIMITED = (226, 80.0)                   # round 1 uses up its budget, leaves no outlier, and round 2 still gains
TWELVE_SEED, NINE_SEED = 86, 86         # M d64 of the chi2 of their round-1 trials stays under the cap


@functools.lru_cache(maxsize=None)
def _seam():
    return make_pack(SEAM_SEED, 513, "pp")


@functools.lru_cache(maxsize=None)
def case(name):
    if name.endswith("-fs"):
        return dict(case(name[:-3]), fix_scale=True)
    if name == "seam-513-rotated":
        return cut(_seam(), rotation_100(513))
    if name.startswith("seam-"):
        return cut(_seam(), np.arange(int(name[5:])))
    if name == "big-1500":
        return make_pack(32, 1500, "pp")
    if name.startswith("cam-"):                         # cam-<c1><c2>-s<scale>: 96 pairs
        _, cams, sc = name.split("-")
        return make_pack(40 + CAMS.index(cams) * 3 + SCALES.index(float(sc[1:])), 96, cams, scale=float(sc[1:]), outlier_frac=0.4, perturb=2.0)
    if name.startswith("norm-"):                        # norm-<c1><c2>: 96 pairs, 24 of them with normalised coordinates as obs2
        return make_pack(80 + CAMS.index(name[5:]), 96, name[5:], n_norm=24)
    if name == "far":                                   # a start 25 times as far off: step rotations of about 0.1 rad
        return make_pack(61, 120, "pp", perturb=25.0, outlier_frac=0.1)
    if name == "near":                                  # a start a 2e-4-th as far off and little noise: step rotations below 1e-5 rad
        return make_pack(62, 120, "pp", perturb=2e-4, noise_px=1e-4, outlier_frac=0.0)
    if name == REJECT[0]:
        return make_pack(int(name[7:]), 40, "pp", perturb=REJECT[1], outlier_frac=0.3)
    if name == "limited":
        return make_pack(LIMITED[0], 64, "pp", perturb=LIMITED[1], outlier_frac=0.0, noise_px=0.3)
    if name == "zero-info":
        pk = dict(case("seam-65"))
        pk["info1"], pk["info2"] = np.zeros(65), np.zeros(65)
        return pk
    if name in ("twelve-2", "twelve-3"):                # 12 pairs with 2 and with 3 gross outliers: 10 and 9 inliers after round 1
        return make_pack(TWELVE_SEED, 12, "pp", outlier_frac=0.0, gross=int(name[-1]), noise_px=0.3, perturb=0.3)
    if name == "nine":                                  # 9 pairs: round 1 only
        return make_pack(NINE_SEED, 9, "pp", outlier_frac=0.0, gross=1, noise_px=0.3, perturb=0.3)
    if name == "converged":
        return _converged()
    raise KeyError(name)


STRICT_HI = float(F32(10.0))
STRICT_LO = float(np.nextafter(F32(10.0), F32(-np.inf)))


@functools.lru_cache(maxsize=None)
def _converged(seed=91, n=64):
    """A pack whose input S12 is the long-double reference's converged robust estimate (th2 = 10), and in which the larger chi2 of one
    pair (pack["strict_pair"]) sits there halfway between the float32 10 and the float32 below it (4.8e-8 relative from either): the
    pair's information is scaled for that and the estimate converged again, until both hold.  One robust iteration from there steps
    about 1e-11 (relative, in that chi2), so the chi2 of its trial is pinned three orders below the gap between the two thresholds,
    in float64 as on the device, and the verdict of the round-1 classification on that pair is decidable."""
    s3.require_extended()
    L = np.longdouble
    pk = make_pack(seed, n, "pp", noise_px=0.05, outlier_frac=0.08)
    target = (L(STRICT_HI) + L(STRICT_LO)) / 2
    r = s3.run(pk, L, (10, 0, 0))
    top = np.maximum(*r.chi2_round1)
    cand = [q for q in np.argsort(top.astype(np.float64)) if 2 < top[q] < 60]
    p = int(cand[len(cand) // 2])
    edge = "info1" if r.chi2_round1[0][p] >= r.chi2_round1[1][p] else "info2"
    S = r.S_round1
    for _ in range(8):
        for _ in range(3):
            S = s3.run(dict(pk, S12=np.asarray(S).astype(np.float64)), L, (10, 0, 0)).S_round1
        c = s3.pair_chi2_at(pk, S, L)[0 if edge == "info1" else 1][p]
        info = pk[edge].copy()
        info[p] = float(L(info[p]) * target / c)
        pk = dict(pk, **{edge: info})
    return dict(pk, S12=np.asarray(S).astype(np.float64), strict_pair=p)


# ------------------------------------------------------------------------------------------------------------- probes
def with_probe(pk, budgets=s3.BUDGETS, th2=None):
    out = dict(pk, iterations=tuple(int(k) for k in budgets))
    if th2 is not None:
        out["th2"] = float(F32(th2))
    return out


def strict_pair(cname, stage):
    """A pair whose larger chi2 at `stage` ("final": at the input S12, probe e; "round1": at the trial of probe r1 of the case
    `converged`) is at least 1e-6 (relative) from every other chi2: (pair, the float32 just above that long-double chi2, the float32
    just below it)."""
    if stage == "round1":                               # the case is built for it: see _converged
        return case(cname)["strict_pair"], STRICT_HI, STRICT_LO
    r = refs(f"{cname}/e").ld
    c12, c21 = r.chi2_12, r.chi2_21
    top = np.maximum(c12, c21)
    allc = np.concatenate([c12, c21])
    order = [p for p in np.argsort(top.astype(np.float64)) if top[p] < 0.9 * TH2]
    for p in order[len(order) // 2:]:
        c = top[p]
        if np.sort(np.abs(allc - c))[1] < 1e-6 * c:
            continue
        hi = F32(c)
        if np.longdouble(hi) <= c:
            hi = np.nextafter(hi, F32(np.inf))
        lo = np.nextafter(hi, F32(-np.inf))
        assert np.longdouble(lo) < c < np.longdouble(hi)
        return int(p), float(hi), float(lo)
    raise AssertionError("no pair qualifies")


def _strict(cname, stage, which):
    _, hi, lo = strict_pair(cname, stage)
    return with_probe(case(cname), (0, 0, 0) if stage == "final" else (1, 0, 0), th2=hi if which == "above" else lo)


PROBE_BUILDERS = {
    "e": lambda cn: with_probe(case(cn), (0, 0, 0)),
    "full": lambda cn: with_probe(case(cn)),
    "b532": lambda cn: with_probe(case(cn), (5, 3, 2)),
    "strict-round1-above": lambda cn: _strict(cn, "round1", "above"),
    "strict-round1-below": lambda cn: _strict(cn, "round1", "below"),
    "strict-final-above": lambda cn: _strict(cn, "final", "above"),
    "strict-final-below": lambda cn: _strict(cn, "final", "below"),
}


@functools.lru_cache(maxsize=None)
def probe(name):
    cname, kind = name.rsplit("/", 1)
    if kind in PROBE_BUILDERS:
        return PROBE_BUILDERS[kind](cname)
    k = int(kind[1:])
    assert kind[0] in "rn"
    return with_probe(case(cname), (k, 0, 0) if kind[0] == "r" else (0, k, k))


def orders(n):
    """The pair orders in which the float64 reference is run: as given, reversed, and two fixed shuffles.  Its distance from long double
    after a few iterations varies thirtyfold with the order of its sums (limited/b532: chi2_end 1.9e-7 .. 5.9e-6), so one order alone
    understates the reference's own error; d64 is the largest of the four.  This widens what a single run would give, so the cause was
    looked for in the kernel first: sim3_linearize sums a thread's pairs p, p + 256, ... in order, then the 64 lanes of a wavefront by
    butterfly, then the four wavefronts in index order, every product unfused (contraction is off in the file).  That is one more order
    of the same float64 sums, no wider and no narrower than the reference's; the device's own results move by as much when its pairs
    are rotated (seam-513-rotated).  What varies is the 1e-7 relative noise of the 1e-9 differences, which the 7x7 solve amplifies.
    The GPU module also prints the worst d_dev against the MEDIAN of the four distances, to show what taking the largest adds."""
    return [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(1).permutation(n), np.random.default_rng(2).permutation(n)]


def _unordered(r, order):
    """A run on cut(pack, order), its per-pair arrays back in the pack's order."""
    def back(a):
        o = np.empty_like(a)
        o[order] = a
        return o
    out = SimpleNamespace(**vars(r))
    for f in ("outlier1", "outlier", "chi2_12", "chi2_21"):
        setattr(out, f, back(getattr(r, f)))
    return out


@functools.lru_cache(maxsize=None)
def refs(name):
    """namespace(ld, f64, f64_orders): long double, float64, and float64 in every order of orders() (the first is f64)."""
    s3.require_extended()
    pk = probe(name)
    runs = [_unordered(s3.run(cut(pk, o), np.float64), o) for o in orders(len(pk["info1"]))]
    return SimpleNamespace(ld=s3.run(pk, np.longdouble), f64=runs[0], f64_orders=runs)


def lin_pack(cname, robust):
    return case(cname) if robust else with_probe(case(cname), th2=s3.PLAIN_TH2)


@functools.lru_cache(maxsize=None)
def lin_refs(cname, robust):
    s3.require_extended()
    pk = case(cname)
    runs = [s3.first_linearization(cut(pk, o), np.float64, robust) for o in orders(len(pk["info1"]))]
    return SimpleNamespace(ld=s3.first_linearization(pk, np.longdouble, robust), f64=runs[0], f64_orders=runs)


def settled(name):
    """A probe's decisions are settled when long double and float64 (in every order) report the same iteration counts and flags."""
    a = refs(name).ld
    return all(np.array_equal(a.iterations, b.iterations) and (a.round2, a.n_bad, a.n_in) == (b.round2, b.n_bad, b.n_in)
               and np.array_equal(a.outlier1, b.outlier1) and np.array_equal(a.outlier, b.outlier) for b in refs(name).f64_orders)


def _budget_left(cname, mode):
    rnd = 0 if mode == "r" else 1
    return min(int(refs(f"{cname}/{mode}10").ld.iterations[rnd]) + 1, 10)


@functools.lru_cache(maxsize=None)
def trajectory_length(cname, mode):
    """K: the first budget that the long-double reference does not use up (10 when it uses every one), cut before the first k at which
    M d64 would pass a cap or float64 and long double part ways on a count or a flag (KannalaBrandt8: the float32 staircase of theta
    and psi makes them part after an iteration or two)."""
    for k in range(1, _budget_left(cname, mode) + 1):
        if not (within_caps(f"{cname}/{mode}{k}") and settled(f"{cname}/{mode}{k}")):
            return k - 1
    return _budget_left(cname, mode)


# the pairs whose obs2 are normalised coordinates are hundreds of pixels off in camera 2 (that is the reference): Huber tames them in
# round 1, which then classifies them out; a plain round over them is far from anything OptimizeSim3 runs, so they get no n<k> probe.
# A single pair leaves H of rank 2, and the step to the damping alone: seam-1 shows in the linearisation only
NORM_CASES = ["norm-pp", "norm-kk", "norm-pk"]
ERROR_CASES = ([f"cam-{c}-s{s}" for c in CAMS for s in SCALES] + NORM_CASES + [f"seam-{n}" for n in SEAM_SIZES if n >= 10]
               + ["big-1500"])
LIN_CASES = ([f"seam-{n}" for n in SEAM_SIZES] + ["big-1500"] + [f"cam-{c}-s1.0" for c in CAMS] + ["cam-pp-s0.5", "cam-kp-s3.0"]
             + NORM_CASES + ["seam-257-fs", "cam-kk-s1.0-fs", "cam-pk-s1.0-fs"])
ONE_ITERATION_PROBES = ([f"{c}/r1" for c in LIN_CASES + ["far", "near"] if c != "seam-1"]
                        + [f"{c}/n1" for c in LIN_CASES + ["far", "near"] if c not in ("seam-1", "seam-9") + tuple(NORM_CASES)])
TRAJECTORY_CASES = ("seam-65", "seam-257", "far", "seam-65-fs", "cam-kk-s1.0", "cam-pk-s1.0", REJECT[0])
STOP_PROBES = ["seam-65/full", "far/full", "seam-65/b532", "limited/b532", "nine/full"]
CLASSIFICATION_PROBES = ([f"seam-65/strict-final-{w}" for w in ("above", "below")] + [f"converged/strict-round1-{w}" for w in ("above", "below")]
                         + ["twelve-2/full", "twelve-3/full"])
STORAGE_PROBES = ["seam-513/full", "seam-513/r3", "seam-513/n3", "big-1500/full"]


# reject-110 is there for its rejected first plain trial; robust, M d64 of its first trial's chi2 is already over the cap, so it has no r
TRAJECTORIES = [(c, m) for c in TRAJECTORY_CASES for m in "rn" if (c, m) != (REJECT[0], "r")]


def trajectory_probes():
    return [f"{c}/{m}{k}" for c, m in TRAJECTORIES for k in range(1, trajectory_length(c, m) + 1)]


def all_probes():
    return sorted(set([f"{c}/e" for c in ERROR_CASES] + ONE_ITERATION_PROBES + trajectory_probes() + STOP_PROBES + CLASSIFICATION_PROBES
                      + STORAGE_PROBES + [f"{REJECT[0]}/n1", "zero-info/full"]))


# ------------------------------------------------------------------------------------------------------------- distances
def _rel(g, r, floor):
    L = np.longdouble
    g, r = np.asarray(g).astype(L), np.asarray(r).astype(L)
    if g.size == 0:
        return 0.0
    return float(np.max(np.abs(g - r) / np.maximum(np.abs(r), L(floor))))


def sim3_distance(g, r):
    """(rotation in rad, relative translation, relative scale) between two Sim3, differences formed in long double."""
    L = np.longdouble
    g, r = np.asarray(g).astype(L), np.asarray(r).astype(L)
    gq, rq = g[:4] / np.sqrt((g[:4] ** 2).sum()), r[:4] / np.sqrt((r[:4] ** 2).sum())
    rel = pn.quat_mul(gq, np.concatenate([-rq[:3], rq[3:4]]))
    rot = float(2 * np.arctan2(np.sqrt((rel[:3] ** 2).sum()), np.abs(rel[3])))
    tr = float(np.sqrt(((g[4:7] - r[4:7]) ** 2).sum()) / max(np.sqrt((r[4:7] ** 2).sum()), L(1e-12)))
    return rot, tr, float(abs(g[7] - r[7]) / r[7])


def distances(name, got):
    """Distance of a result of probe `name` (device or float64 reference) from the long-double reference, each relative to its quantity:
    pair_chi2   both edges' chi2 of the pairs that were last evaluated at the exported S12, against the long-double chi2 AT THE S12 THAT
                `got` EXPORTS, relative to max(chi2, 1e-3), worst pair: this is exact arithmetic's answer to the result's own estimate
    trial_chi2  the chi2 of the other evaluated pairs (at an estimate that is not exported), against the reference's run, relative to
                max(chi2, 1)
    chi2_end    per round, relative;  rot (rad), trans, scale (relative): S12 against the reference's run."""
    ld = refs(name).ld
    d = {}
    at, ot = ld.at_S, ld.evaluated & ~ld.at_S
    if at.any():
        c12, c21 = s3.pair_chi2_at(probe(name), np.asarray(got.S12), np.longdouble)
        d["pair_chi2"] = max(_rel(np.asarray(got.chi2_12)[at], c12[at], 1e-3), _rel(np.asarray(got.chi2_21)[at], c21[at], 1e-3))
    if ot.any():
        d["trial_chi2"] = max(_rel(np.asarray(got.chi2_12)[ot], ld.chi2_12[ot], 1.0), _rel(np.asarray(got.chi2_21)[ot], ld.chi2_21[ot], 1.0))
    g, r = np.asarray(got.chi2_end).astype(np.longdouble), ld.chi2_end
    d["chi2_end"] = float(np.max(np.abs(g - r) / np.where(r != 0, np.abs(r), np.longdouble(1))))
    d["rot"], d["trans"], d["scale"] = sim3_distance(got.S12, ld.S12)
    return d


@functools.lru_cache(maxsize=None)
def bounds(name):
    """Per quantity: (d64, bound) with d64 the float64 reference's distance from the long-double one (the largest over orders()) and
    bound = max(M d64, FLOOR)."""
    ds = _d64s(name)
    return {k: (max(d[k] for d in ds), max(M * max(d[k] for d in ds), FLOOR)) for k in ds[0]}


@functools.lru_cache(maxsize=None)
def _d64s(name):
    return [distances(name, r) for r in refs(name).f64_orders]


def d64_median(name):
    """Per quantity the median of the four float64 distances: printed beside the largest, to show what taking the largest adds."""
    return {k: float(np.median([d[k] for d in _d64s(name)])) for k in _d64s(name)[0]}


def within_caps(name):
    return all(M * d64 <= CAPS[k] for k, (d64, _) in bounds(name).items())


def lin_distances(H, b, chi, ld):
    """Scaled distances of a linearisation from the long-double one: H entry by entry over s_i s_j, s_i = sqrt(max(H_ii, 1e-12 max
    diag)) of the reference, b over s_i sqrt(chi2), chi2 relative."""
    L = np.longdouble
    diag = np.diag(ld.H)
    s = np.sqrt(np.maximum(diag, L(1e-12) * diag.max()))
    dH = float(np.max(np.abs(np.asarray(H).astype(L) - ld.H) / np.outer(s, s)))
    db = float(np.max(np.abs(np.asarray(b).astype(L) - ld.b) / (s * np.sqrt(ld.chi))))
    return dict(H=dH, b=db, chi2=float(abs(L(chi) - ld.chi) / ld.chi))


@functools.lru_cache(maxsize=None)
def lin_bounds(cname, robust):
    r = lin_refs(cname, robust)
    ds = _lin_d64s(cname, robust)
    return {k: (max(d[k] for d in ds), max(M * max(d[k] for d in ds), FLOOR)) for k in ds[0]}


@functools.lru_cache(maxsize=None)
def _lin_d64s(cname, robust):
    r = lin_refs(cname, robust)
    return [lin_distances(f.H, f.b, f.chi, r.ld) for f in r.f64_orders]


def lin_d64_median(cname, robust):
    ds = _lin_d64s(cname, robust)
    return {k: float(np.median([d[k] for d in ds])) for k in ds[0]}


def rounding_mismatches(cname):
    """Pairs of a KannalaBrandt8 case whose float32 roundings (x2 + y2, its root, Z, theta, psi) at the input S12 or at one of its 14
    perturbed states differ between the float64 and the long-double run: the only pairs a comparison of H, b or a chi2 may leave out."""
    pk = case(cname)
    a, b = s3.linearization_roundings(pk, np.float64), s3.linearization_roundings(pk, np.longdouble)
    bad = np.zeros(len(pk["info1"]), bool)
    for x, y in zip(a, b):
        if x is not None:
            bad |= np.any(x != y, axis=(0, 2))
    return np.flatnonzero(bad)
