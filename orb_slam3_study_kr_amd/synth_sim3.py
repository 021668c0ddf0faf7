"""Seeded keyframe pairs for Optimizer::OptimizeSim3, and a Python restatement of its pair walk.

make_case() draws two keyframes whose cameras see the same points through a known relative Sim3 S12 (x1 = S12 x2), keypoints
with pixel noise, a fraction of swapped matches (outliers), and optionally pairs whose second point has no keypoint in pKF2
(i2 < 0), bad map points, NULL map points of pKF1, second points behind pKF2's camera, fixed or free scale, and Pinhole or
KannalaBrandt8 cameras.  host_input() turns a case into the stand-in input of the test-only host library (osh_host_sim3_input),
pack() restates the walk of src/Optimizer.cc:2162-2277 on the same float data, and problem() builds an osh_sim3_problem from a
pack (its budgets from the pack's "iterations" when present, else ITERATIONS).  Sim3 arrays are qx qy qz qw tx ty tz s.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi

F32 = np.float32
TH2 = 10.0   # LoopClosing's th2 for OptimizeSim3 (src/LoopClosing.cc:558, :768)
ITERATIONS = (5, 10, 5)   # optimize(5), then optimize(nBad > 0 ? 10 : 5): osh_sim3_problem.iterations


def _quat_from_axis_angle(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    a = w / th
    return np.concatenate([a * np.sin(th / 2), [np.cos(th / 2)]])


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def sim3_apply(S, X):
    """s R X + t for X [..., 3] (plain float64, for generating data)."""
    return S[7] * (X @ _quat_to_R(S[:4]).T) + S[4:7]


def sim3_apply_inverse(S, X):
    return ((X - S[4:7]) @ _quat_to_R(S[:4])) / S[7]


def project_f64(cam, kb8, X):
    """Pixel of camera-frame points X [n, 3] (plain float64, for generating observations)."""
    if not kb8:
        return np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], -1)
    th = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2])
    psi = np.arctan2(X[:, 1], X[:, 0])
    r = th + cam[4] * th ** 3 + cam[5] * th ** 5 + cam[6] * th ** 7 + cam[7] * th ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], -1)


PINHOLE = np.array([458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0])
KB8 = np.array([190.978, 190.973, 254.932, 256.897, 0.00348238, 0.000715034, -0.00205323, 0.000202937])


@dataclass
class Sim3Case:
    kf1: dict
    kf2: dict
    mp_pos: np.ndarray            # [P, 3] float32
    mp_bad: np.ndarray            # [P] uint8
    mp_index2: np.ndarray         # [P] int32
    mp_track_level: np.ndarray    # [P] int32
    kf1_mp: np.ndarray            # [N1] int32
    matches1: np.ndarray          # [N1] int32
    S12_true: np.ndarray
    S12: np.ndarray               # initial estimate
    th2: float = TH2
    fix_scale: bool = False
    all_points: bool = True
    X1c_true: np.ndarray = None   # [N1, 3] exact camera-1 points of the pair slots (float64)
    _keep: list = field(default_factory=list)


def _keyframe(pose_qt, cam, kb8, keys, octave, n_levels=8, scale=1.2):
    inv = (1.0 / (scale ** (2 * np.arange(n_levels)))).astype(F32)
    return dict(pose=np.asarray(pose_qt, F32), cam=np.asarray(cam, F32), kb8=int(kb8), keys_un=np.ascontiguousarray(keys, F32),
                octave=np.ascontiguousarray(octave, np.int32), inv_level_sigma2=inv)


def make_case(seed=0, n_pairs=300, outlier_frac=0.1, n_no_i2=0, n_bad=0, n_null_mp1=0, n_neg_depth=0, fix_scale=False,
              kb8=False, noise_px=0.7, all_points=True, init_perturb=1.0) -> Sim3Case:
    """A keyframe pair with n_pairs candidate matches plus the special slots asked for (each kind takes its own slots)."""
    rng = np.random.default_rng(seed)
    cam = KB8 if kb8 else PINHOLE
    scale = 1.0 if fix_scale else float(rng.uniform(0.7, 1.4))
    q12 = _quat_from_axis_angle(rng.normal(size=3) * 0.08)
    S12_true = np.concatenate([q12, rng.normal(size=3) * 0.15, [scale]])
    # initial estimate: the true S12 a little off (as Sim3Solver leaves it)
    dq = _quat_from_axis_angle(rng.normal(size=3) * 0.004 * init_perturb)
    S12 = np.concatenate([_quat_mul(dq, q12), S12_true[4:7] + rng.normal(size=3) * 0.01 * init_perturb,
                          [scale if fix_scale else scale * (1 + 0.01 * init_perturb * rng.normal())]])
    S12[:4] /= np.linalg.norm(S12[:4])
    N1 = n_pairs + n_no_i2 + n_bad + n_null_mp1 + n_neg_depth
    # camera-1 points in front of both cameras
    if kb8:
        d = rng.normal(size=(N1, 3)); d[:, 2] = np.abs(d[:, 2]) + 0.6
    else:
        d = np.stack([rng.uniform(-0.6, 0.6, N1), rng.uniform(-0.45, 0.45, N1), np.ones(N1)], -1)
    X1c = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 8.0, (N1, 1))
    X2c = sim3_apply_inverse(S12_true, X1c)
    neg = np.arange(N1 - n_neg_depth, N1)
    X2c[neg, 2] = -np.abs(X2c[neg, 2])               # behind pKF2's camera
    # keyframe poses (world -> camera)
    qa, qb = (_quat_from_axis_angle(rng.normal(size=3) * 0.5) for _ in range(2))
    ta, tb = rng.normal(size=3), rng.normal(size=3)
    T1 = np.concatenate([qa, ta]).astype(F32).astype(np.float64)
    T2 = np.concatenate([qb, tb]).astype(F32).astype(np.float64)
    P1w = (X1c - T1[4:7]) @ _quat_to_R(T1[:4])
    P2w = (X2c - T2[4:7]) @ _quat_to_R(T2[:4])
    # keypoints: pKF1 slot i = pair i; pKF2 keypoints in a shuffled order
    n_levels = 8
    kp1 = project_f64(cam, kb8, X1c) + rng.normal(size=(N1, 2)) * noise_px
    oct1 = rng.integers(0, n_levels, N1)
    perm = rng.permutation(N1)                        # pair i -> keypoint perm[i] of pKF2
    kp2 = np.zeros((N1, 2)); oct2 = rng.integers(0, n_levels, N1)
    with np.errstate(all="ignore"):
        kp2[perm] = project_f64(cam, kb8, np.where(X2c[:, 2:3] > 0, X2c, 1.0)) + rng.normal(size=(N1, 2)) * noise_px
    kf1 = _keyframe(T1, cam, kb8, kp1, oct1, n_levels)
    kf2 = _keyframe(T2, cam, kb8, kp2, oct2, n_levels)
    # map points: 0..N1-1 the pKF1 points, N1..2N1-1 the matched pKF2 points
    mp_pos = np.concatenate([P1w, P2w]).astype(F32)
    mp_bad = np.zeros(2 * N1, np.uint8)
    mp_index2 = np.full(2 * N1, -1, np.int32)
    mp_index2[N1:] = perm
    track = rng.integers(0, n_levels, 2 * N1).astype(np.int32)
    kf1_mp = np.arange(N1, dtype=np.int32)
    matches1 = (N1 + np.arange(N1)).astype(np.int32)
    slot = n_pairs
    no_i2 = np.arange(slot, slot + n_no_i2); slot += n_no_i2
    mp_index2[N1 + no_i2] = -1
    bad = np.arange(slot, slot + n_bad); slot += n_bad
    for k, i in enumerate(bad):                       # alternate: the pKF1 point or the matched point is bad
        mp_bad[i if k % 2 == 0 else N1 + i] = 1
    null1 = np.arange(slot, slot + n_null_mp1); slot += n_null_mp1
    kf1_mp[null1] = -1
    # swapped matches among the regular pairs
    n_out = int(round(outlier_frac * n_pairs))
    if n_out >= 2:
        sw = rng.choice(n_pairs, n_out, replace=False)
        matches1[sw] = matches1[np.roll(sw, 1)]
    # a few slots without a match at all
    empty = rng.choice(n_pairs, max(1, n_pairs // 50), replace=False) if n_pairs >= 20 else np.array([], int)
    matches1[empty] = -1
    return Sim3Case(kf1=kf1, kf2=kf2, mp_pos=mp_pos, mp_bad=mp_bad, mp_index2=mp_index2, mp_track_level=track, kf1_mp=kf1_mp,
                    matches1=matches1, S12_true=S12_true, S12=S12, fix_scale=fix_scale, all_points=all_points, X1c_true=X1c)


def host_input(case: Sim3Case) -> capi.HostSim3Input:
    """osh_host_sim3_input of a case (the case keeps the arrays alive)."""
    def kf(d):
        k = capi.HostSim3Kf()
        k.pose[:] = [float(v) for v in d["pose"]]
        k.cam[:] = [float(v) for v in d["cam"]]
        k.kb8 = d["kb8"]; k.n_keys = len(d["octave"])
        k.keys_un = capi.ptr(d["keys_un"], capi.c_float_p); k.octave = capi.ptr(d["octave"], capi.c_int32_p)
        k.n_levels = len(d["inv_level_sigma2"]); k.inv_level_sigma2 = capi.ptr(d["inv_level_sigma2"], capi.c_float_p)
        return k
    s = capi.HostSim3Input()
    s.kf1 = kf(case.kf1); s.kf2 = kf(case.kf2)
    s.n_points = len(case.mp_bad)
    s.mp_pos = capi.ptr(case.mp_pos, capi.c_float_p); s.mp_bad = capi.ptr(case.mp_bad, capi.c_uint8_p)
    s.mp_index2 = capi.ptr(case.mp_index2, capi.c_int32_p); s.mp_track_level = capi.ptr(case.mp_track_level, capi.c_int32_p)
    s.kf1_mp = capi.ptr(case.kf1_mp, capi.c_int32_p)
    s.n_matches = len(case.matches1); s.matches1 = capi.ptr(case.matches1, capi.c_int32_p)
    s.S12[:] = [float(v) for v in case.S12]
    s.th2 = case.th2; s.fix_scale = int(case.fix_scale); s.all_points = int(case.all_points)
    return s


def _se3f_apply(pose, P):
    """Sophus SE3f * p in float32 as the stand-in header states it: v + w uv + vec x uv, uv = 2 vec x v, then + t."""
    x, y, z, w = (F32(v) for v in pose[:4])
    px, py, pz = P
    two = F32(2)
    uvx, uvy, uvz = two * (y * pz - z * py), two * (z * px - x * pz), two * (x * py - y * px)
    return (px + w * uvx + (y * uvz - z * uvy) + F32(pose[4]), py + w * uvy + (z * uvx - x * uvz) + F32(pose[5]),
            pz + w * uvz + (x * uvy - y * uvx) + F32(pose[6]))


def pack(case: Sim3Case) -> dict:
    """The pair walk of OptimizeSim3 restated: index, X1c, X2c, obs1, obs2, info1, info2 and the cameras."""
    out = dict(index=[], X1c=[], X2c=[], obs1=[], obs2=[], info1=[], info2=[])
    N1 = len(case.matches1)
    for i in range(N1):
        m2 = int(case.matches1[i])
        if m2 < 0:
            continue
        m1 = int(case.kf1_mp[i]) if i < len(case.kf1_mp) else -1
        i2 = int(case.mp_index2[m2])
        if m1 < 0:
            continue                                   # NULL pMP1: pMP2's vertex only, no edge
        if case.mp_bad[m1] or case.mp_bad[m2]:
            continue
        P1 = _se3f_apply(case.kf1["pose"], case.mp_pos[m1])
        P2 = _se3f_apply(case.kf2["pose"], case.mp_pos[m2])
        if i2 < 0 and not case.all_points:
            continue
        if P2[2] < 0:
            continue
        out["index"].append(i)
        out["X1c"].append([float(v) for v in P1]); out["X2c"].append([float(v) for v in P2])
        out["obs1"].append([float(v) for v in case.kf1["keys_un"][i]])
        out["info1"].append(float(case.kf1["inv_level_sigma2"][case.kf1["octave"][i]]))
        if i2 >= 0:
            out["obs2"].append([float(v) for v in case.kf2["keys_un"][i2]])
            oct2 = int(case.kf2["octave"][i2])
        else:
            invz = F32(1) / P2[2]
            out["obs2"].append([float(P2[0] * invz), float(P2[1] * invz)])
            oct2 = 0                                   # cv::KeyPoint(pt, size = mnTrackScaleLevel): octave stays 0
        out["info2"].append(float(case.kf2["inv_level_sigma2"][oct2]))
    res = {k: np.asarray(v, np.float64) for k, v in out.items() if k != "index"}
    res["index"] = np.asarray(out["index"], np.int32)
    n = len(res["index"])
    for k, w in (("X1c", 3), ("X2c", 3), ("obs1", 2), ("obs2", 2)):
        res[k] = res[k].reshape(n, w)
    res["cam1"] = np.zeros(8); res["cam2"] = np.zeros(8)
    w1 = 8 if case.kf1["kb8"] else 4
    w2 = 8 if case.kf2["kb8"] else 4
    res["cam1"][:w1] = case.kf1["cam"][:w1].astype(np.float64)
    res["cam2"][:w2] = case.kf2["cam"][:w2].astype(np.float64)
    res["kb8_1"], res["kb8_2"] = case.kf1["kb8"], case.kf2["kb8"]
    res["S12"] = np.asarray(case.S12, np.float64)
    res["fix_scale"] = bool(case.fix_scale)
    res["th2"] = float(F32(case.th2))
    return res


def exact_pack(case: Sim3Case) -> dict:
    """A pack of the regular pairs with float64 points and noiseless float64 observations of S12_true (for recovery tests)."""
    n = len(case.X1c_true)
    X1 = np.ascontiguousarray(case.X1c_true)
    X2 = sim3_apply_inverse(case.S12_true, X1)
    keep = X2[:, 2] > 0
    X1, X2 = X1[keep], X2[keep]
    cam = case.kf1["cam"].astype(np.float64)
    kb = case.kf1["kb8"]
    return dict(index=np.arange(n, dtype=np.int32)[keep], X1c=X1, X2c=X2, obs1=project_f64(cam, kb, sim3_apply(case.S12_true, X2)),
                obs2=project_f64(cam, kb, X2), info1=np.ones(len(X1)), info2=np.ones(len(X1)),
                cam1=np.where(np.arange(8) < (8 if kb else 4), cam, 0.0), cam2=np.where(np.arange(8) < (8 if kb else 4), cam, 0.0),
                kb8_1=kb, kb8_2=kb, S12=np.asarray(case.S12, np.float64), fix_scale=bool(case.fix_scale), th2=float(F32(case.th2)))


def problem(pk: dict, keep: list | None = None) -> capi.Sim3Problem:
    """osh_sim3_problem of a pack (arrays made contiguous and kept alive in `keep`, or in the pack)."""
    keep = pk.setdefault("_keep", []) if keep is None else keep
    p = capi.Sim3Problem()
    p.n_pairs = len(pk["index"])
    p.S12[:] = [float(v) for v in pk["S12"]]
    p.fix_scale = int(pk["fix_scale"]); p.th2 = pk["th2"]
    p.cam1[:] = [float(v) for v in pk["cam1"]]; p.cam2[:] = [float(v) for v in pk["cam2"]]
    p.kb8_1 = int(pk["kb8_1"]); p.kb8_2 = int(pk["kb8_2"])
    p.iterations[:] = [int(v) for v in pk.get("iterations", ITERATIONS)]
    for k in ("X1c", "X2c", "obs1", "obs2", "info1", "info2"):
        a = np.ascontiguousarray(pk[k], np.float64)
        keep.append(a)
        setattr(p, k, capi.ptr(a, capi.c_double_p))
    return p


@dataclass
class Sim3ResultArrays:
    S12: np.ndarray
    outlier1: np.ndarray
    outlier: np.ndarray
    chi2_12: np.ndarray
    chi2_21: np.ndarray
    n_bad: int
    n_in: int
    round2: bool
    iterations: tuple
    chi2_end: tuple


def bind_result(n_pairs: int):
    """An osh_sim3_result with arrays for n_pairs and the arrays themselves."""
    arrs = dict(outlier1=np.zeros(n_pairs, np.uint8), outlier=np.zeros(n_pairs, np.uint8), chi2_12=np.zeros(n_pairs),
                chi2_21=np.zeros(n_pairs))
    r = capi.Sim3Result()
    r.outlier1 = capi.ptr(arrs["outlier1"], capi.c_uint8_p); r.outlier = capi.ptr(arrs["outlier"], capi.c_uint8_p)
    r.chi2_12 = capi.ptr(arrs["chi2_12"], capi.c_double_p); r.chi2_21 = capi.ptr(arrs["chi2_21"], capi.c_double_p)
    return r, arrs


def read_result(r: capi.Sim3Result, arrs: dict) -> Sim3ResultArrays:
    return Sim3ResultArrays(S12=np.array(r.S12[:]), n_bad=r.n_bad, n_in=r.n_in, round2=bool(r.round2), iterations=tuple(r.iterations),
                            chi2_end=tuple(r.chi2_end), **{k: v.copy() for k, v in arrs.items()})
