"""Seeded keyframe maps with a loop closure for Optimizer::OptimizeEssentialGraph, and a Python restatement of its graph walk.

make_map() lays keyframes on a circle, accumulates rotation, translation and (monocular) scale drift along the chain, and
closes the loop between the newest keyframe and one of the first: a parent tree, covisibility weights above and below 100,
CorrectedSim3 / NonCorrectedSim3 / LoopConnections of the current keyframe's neighbourhood, optional earlier loop edges,
inertial chains and map points with reference keyframes.  pack_loop() / pack_merge() restate the edge rules of
src/Optimizer.cc:1501-1711 and :1786-2040 so that tests can check the host layer's graph walk, and build_host_map() turns a map
into the stand-in objects of the test-only host library.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi
from .pgo import INFO_4DOF, Pgo4Graph, PgoGraph

MIN_FEAT = 100


# ---- Sim3 arithmetic of the graph walk (g2o::Sim3 product / inverse as the stand-in header states them) ----
def _quat_rotate(q, v):
    x, y, z, w = q
    uv = np.array([y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]])
    uv = uv + uv
    return np.array([v[0] + w * uv[0] + (y * uv[2] - z * uv[1]), v[1] + w * uv[1] + (z * uv[0] - x * uv[2]),
                     v[2] + w * uv[2] + (x * uv[1] - y * uv[0])])


def sim3_mul(a, b):
    ax, ay, az, aw = a[:4]
    bx, by, bz, bw = b[:4]
    q = [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
         aw * bw - ax * bx - ay * by - az * bz]
    r = _quat_rotate(a[:4], b[4:7])
    return np.array(q + [a[7] * r[0] + a[4], a[7] * r[1] + a[5], a[7] * r[2] + a[6], a[7] * b[7]])


def sim3_inverse(a):
    qc = np.array([-a[0], -a[1], -a[2], a[3]])
    f = -1.0 / a[7]
    t = _quat_rotate(qc, np.array([f * a[4], f * a[5], f * a[6]]))
    return np.concatenate([qc, t, [1.0 / a[7]]])


def sim3_from_pose(qt):
    """g2o::Sim3(Tcw.unit_quaternion(), Tcw.translation(), 1.0) from a float pose qx qy qz qw tx ty tz."""
    return np.concatenate([np.asarray(qt, dtype=np.float32).astype(np.float64), [1.0]])


def _rot_to_quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    q = np.array([x, y, z, w])
    return q / np.linalg.norm(q)


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


@dataclass
class SynthPgoMap:
    kf_id: np.ndarray                    # [n] int64 mnId
    pose_qt: np.ndarray                  # [n, 7] float32 Tcw (drifted: the map before the correction)
    true_qt: np.ndarray                  # [n, 7] float64 ground truth Tcw
    parent: np.ndarray                   # [n] int32 (-1: none)
    cov: list                            # per keyframe: list of (other index, weight), any order
    loop_edges: list                     # pairs (a, b) of GetLoopEdges
    prev_kf: np.ndarray                  # [n] int32
    b_imu: np.ndarray                    # [n] bool
    bad: np.ndarray                      # [n] bool
    mp_pos: np.ndarray                   # [m, 3] float32
    mp_ref: np.ndarray                   # [m] int32 reference keyframe index
    mp_corrected_by: np.ndarray          # [m] int64 mnCorrectedByKF
    mp_corrected_ref: np.ndarray         # [m] int64 mnCorrectedReference
    init_index: int = 0
    cur: int = 0
    loop: int = 0
    fix_scale: bool = False
    corrected: dict = field(default_factory=dict)      # index -> Sim3 [8]  (CorrectedSim3)
    noncorrected: dict = field(default_factory=dict)   # index -> Sim3 [8]  (NonCorrectedSim3)
    connections: dict = field(default_factory=dict)    # index -> set of indices (LoopConnections)
    before_merge: dict = field(default_factory=dict)   # index -> float32 qt (mTcwBefMerge)

    @property
    def n(self):
        return len(self.kf_id)

    def weight(self, i, j):
        for o, w in self.cov[i]:
            if o == j:
                return w
        return 0

    def covisibles_by_weight(self, i, w):
        """KeyFrame::GetCovisiblesByWeight: the prefix of the descending (stable) weight order with weights >= w."""
        ordered = sorted(self.cov[i], key=lambda e: -e[1])
        out = []
        for o, wt in ordered:
            if wt < w:
                break
            out.append(o)
        return out

    def children(self, i):
        return {k for k in range(self.n) if self.parent[k] == i}

    def loop_set(self, i):
        s = set()
        for a, b in self.loop_edges:
            if a == i:
                s.add(b)
            if b == i:
                s.add(a)
        return s


def make_map(n_kf: int, seed: int = 0, mono: bool = True, earlier_loop: bool = False, imu: bool = False, n_points: int = 0,
             id_gap: bool = True, neighbourhood: int = 4, band: int = 6) -> SynthPgoMap:
    rng = np.random.default_rng(seed)
    n = n_kf
    radius = max(2.0, 0.05 * n)
    theta = 2 * np.pi * np.arange(n) / n
    Rwc, cw = [], []
    for th in theta:
        yaw = -th
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        Rwc.append(R)
        cw.append(np.array([radius * np.cos(th), 0.1 * np.sin(3 * th), radius * np.sin(th)]))
    # drifted chain: the true relative motions with a rotation bias, noise and (monocular) a growing scale
    Rd, cd, sdrift = [Rwc[0]], [cw[0]], [1.0]
    for i in range(1, n):
        Rrel = Rwc[i - 1].T @ Rwc[i]
        trel = Rwc[i - 1].T @ (cw[i] - cw[i - 1])
        Rrel = Rrel @ _rodrigues(np.array([0.0, 0.6 / n, 0.0]) + rng.normal(0, 0.002, 3))
        s = sdrift[-1] * (1 + (0.15 / n if mono else 0.0))
        trel = trel * (s if mono else 1.0) + rng.normal(0, 0.002, 3)
        Rd.append(Rd[-1] @ Rrel)
        cd.append(cd[-1] + Rd[-2] @ trel)
        sdrift.append(s)
    pose_qt = np.zeros((n, 7), dtype=np.float32)
    true_qt = np.zeros((n, 7))
    for i in range(n):
        Rcw = Rd[i].T
        pose_qt[i, :4] = _rot_to_quat(Rcw)
        pose_qt[i, 4:] = -Rcw @ cd[i]
        Rt = Rwc[i].T
        true_qt[i, :4] = _rot_to_quat(Rt)
        true_qt[i, 4:] = -Rt @ cw[i]
    if id_gap:
        kf_id = np.array([i + i // 5 for i in range(n)], dtype=np.int64)
    else:
        kf_id = np.arange(n, dtype=np.int64)
    parent = np.arange(n, dtype=np.int32) - 1
    cov = [[] for _ in range(n)]

    def connect(a, b, w):
        cov[a] = [(o, x) for o, x in cov[a] if o != b] + [(b, w)]
        cov[b] = [(o, x) for o, x in cov[b] if o != a] + [(a, w)]

    for i in range(n):
        for d in range(1, band + 1):
            if i + d < n:
                connect(i, i + d, int(260 - 30 * d + rng.integers(-10, 11)))
    cur, loop = n - 1, 1
    near_cur = list(range(n - 1, n - 1 - neighbourhood, -1))
    near_loop = list(range(0, neighbourhood + 1))
    m = SynthPgoMap(kf_id=kf_id, pose_qt=pose_qt, true_qt=true_qt, parent=parent, cov=cov, loop_edges=[],
                    prev_kf=(np.arange(n, dtype=np.int32) - 1) if imu else -np.ones(n, dtype=np.int32),
                    b_imu=np.arange(n) >= 1 if imu else np.zeros(n, dtype=bool), bad=np.zeros(n, dtype=bool),
                    mp_pos=np.zeros((0, 3), np.float32), mp_ref=np.zeros(0, np.int32), mp_corrected_by=np.zeros(0, np.int64),
                    mp_corrected_ref=np.zeros(0, np.int64), init_index=0, cur=cur, loop=loop, fix_scale=not mono)
    # the loop: corrected poses of the current keyframe's neighbourhood (ground truth, the map's scale for monocular)
    for a in near_cur:
        s = 1.0 / sdrift[a] if mono else 1.0
        m.corrected[a] = np.concatenate([true_qt[a, :4], s * true_qt[a, 4:], [s]])
        m.noncorrected[a] = sim3_from_pose(pose_qt[a])
        conns = set()
        for b in near_loop:
            w = int(rng.integers(40, 250))
            if a == cur and b == loop:
                w = 60                      # below minFeat: kept by the (pCurKF, pLoopKF) exception
            connect(a, b, w)
            conns.add(b)
        m.connections[a] = conns
    # a parent that is also a loop connection
    m.connections[near_cur[1]].add(int(parent[near_cur[1]]))
    connect(near_cur[1], int(parent[near_cur[1]]), 180)
    if earlier_loop:
        a, b = n // 2, 2
        m.loop_edges.append((a, b))
        m.loop_edges.append((3 * n // 4, n // 4))
    if n_points:
        m.mp_ref = rng.integers(0, n, n_points).astype(np.int32)
        pos = np.zeros((n_points, 3))
        for k, r in enumerate(m.mp_ref):
            pos[k] = cd[r] + Rd[r] @ np.array([rng.normal(0, 1), rng.normal(0, 0.5), 3 + rng.random() * 4])
        m.mp_pos = pos.astype(np.float32)
        m.mp_corrected_by = np.zeros(n_points, np.int64)
        m.mp_corrected_ref = np.zeros(n_points, np.int64)
        for k, r in enumerate(m.mp_ref):
            if r in near_cur and rng.random() < 0.7:
                m.mp_corrected_by[k] = kf_id[cur]
                m.mp_corrected_ref[k] = kf_id[near_cur[int(rng.integers(0, len(near_cur)))]]
    return m


def make_merge(n_kf: int, seed: int = 0, n_points: int = 0):
    """A map for the merge overload: the newest keyframes fixed (good poses), the first ones fixed and corrected (mTcwBefMerge
    = their drifted pose, their pose = ground truth), the rest free.  Returns (map, fixed, fixed_corrected, non_fixed, mps)."""
    m = make_map(n_kf, seed, mono=False, n_points=n_points)
    n = m.n
    fixed = list(range(n - 5, n))
    fixed_corrected = list(range(0, 5))
    non_fixed = list(range(5, n - 5)) + [2]          # keyframe 2 also in the corrected list: skipped as in the reference
    for i in fixed_corrected:
        m.before_merge[i] = m.pose_qt[i].copy()
        m.pose_qt[i] = m.true_qt[i].astype(np.float32)
    mps = list(range(len(m.mp_ref)))
    return m, fixed, fixed_corrected, non_fixed, mps


# ---- restatement of the graph walk ----
def _vertices(m: SynthPgoMap, entries, kf_pose):
    """entries: (index, Sim3, fixed, fix_scale) in insertion order; vertices sorted by mnId, a repeated id keeps the first."""
    order = sorted(range(len(entries)), key=lambda k: (m.kf_id[entries[k][0]], k))
    vof, est, fx, fs, kfs = {}, [], [], [], []
    for k in order:
        i, S, f, s = entries[k]
        if i in vof:
            continue
        vof[i] = len(kfs)
        kfs.append(i)
        est.append(S)
        fx.append(f)
        fs.append(s)
    return vof, np.array(est).reshape(-1, 8), np.array(fx, bool), np.array(fs, bool), kfs


def pack_loop(m: SynthPgoMap, kf_pose=None):
    """src/Optimizer.cc:1501-1711 on the synthetic map: (PgoGraph, vertex keyframe indices, vScw by index)."""
    pose = m.pose_qt if kf_pose is None else kf_pose
    vScw = {}
    entries = []
    for i in range(m.n):
        if m.bad[i]:
            continue
        vScw[i] = m.corrected[i] if i in m.corrected else sim3_from_pose(pose[i])
        entries.append((i, vScw[i], m.kf_id[i] == m.kf_id[m.init_index], m.fix_scale))
    vof, est, fx, fs, kfs = _vertices(m, entries, pose)
    edges, meas = [], []

    def add(i, j, S):
        if i in vof and j in vof:
            edges.append((vof[i], vof[j]))
            meas.append(S)

    def nc(k):
        return m.noncorrected[k] if k in m.noncorrected else vScw.get(k, np.array([0, 0, 0, 1, 0, 0, 0, 1.0]))

    inserted = set()
    for i in sorted(m.connections):
        Swi = sim3_inverse(vScw[i])
        for j in sorted(m.connections[i]):
            if (i != m.cur or j != m.loop) and m.weight(i, j) < MIN_FEAT:
                continue
            add(i, j, sim3_mul(vScw[j], Swi))
            inserted.add((min(m.kf_id[i], m.kf_id[j]), max(m.kf_id[i], m.kf_id[j])))
    for i in range(m.n):
        Swi = sim3_inverse(m.noncorrected[i]) if i in m.noncorrected else sim3_inverse(vScw.get(i, np.array([0, 0, 0, 1, 0, 0, 0, 1.0])))
        p = int(m.parent[i])
        if p >= 0:
            add(i, p, sim3_mul(nc(p), Swi))
        for L in sorted(m.loop_set(i)):
            if m.kf_id[L] < m.kf_id[i]:
                add(i, L, sim3_mul(nc(L), Swi))
        ch = m.children(i)
        for k in m.covisibles_by_weight(i, MIN_FEAT):
            if k != p and k not in ch and not m.bad[k] and m.kf_id[k] < m.kf_id[i]:
                if (min(m.kf_id[i], m.kf_id[k]), max(m.kf_id[i], m.kf_id[k])) in inserted:
                    continue
                add(i, k, sim3_mul(nc(k), Swi))
        if m.b_imu[i] and m.prev_kf[i] >= 0:
            add(i, int(m.prev_kf[i]), sim3_mul(nc(int(m.prev_kf[i])), Swi))
    g = PgoGraph(est, fx, fs, np.array(edges, np.int32).reshape(-1, 2), np.array(meas).reshape(-1, 8))
    return g, kfs, vScw


def pack_merge(m: SynthPgoMap, fixed, fixed_corrected, non_fixed, kf_pose=None):
    """src/Optimizer.cc:1786-2040 on the synthetic map: (PgoGraph, vertex keyframe indices, vScw, vCorrectedSwc, good, bad)."""
    pose = m.pose_qt if kf_pose is None else kf_pose
    I = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    vScw, vCorr, good, badp = {}, {}, {}, {}
    entries = []
    for i in fixed:
        if m.bad[i]:
            continue
        S = sim3_from_pose(pose[i])
        vCorr[i] = sim3_inverse(S)
        entries.append((i, S, True, True))
        good[i], badp[i] = True, False
    ids = set()
    for i in fixed_corrected:
        if m.bad[i]:
            continue
        S = sim3_from_pose(pose[i])
        vCorr[i] = sim3_inverse(S)
        vScw[i] = sim3_from_pose(m.before_merge[i])
        entries.append((i, S, True, False))
        ids.add(i)
        good[i], badp[i] = True, True
    for i in non_fixed:
        if m.bad[i] or i in ids:
            continue
        S = sim3_from_pose(pose[i])
        vScw[i] = S
        entries.append((i, S, False, False))
        ids.add(i)
        good[i], badp[i] = False, True
    vof, est, fx, fs, kfs = _vertices(m, entries, pose)
    allk = list(fixed) + list(fixed_corrected) + list(non_fixed)
    sk = set(allk)
    edges, meas = [], []

    def add(i, j, S):
        if i in vof and j in vof:
            edges.append((vof[i], vof[j]))
            meas.append(S)

    def rel(i, j):
        if good.get(i, False) and good.get(j, False):
            return sim3_inverse(vCorr.get(j, I))
        if badp.get(i, False) and badp.get(j, False):
            return vScw.get(j, I)
        return None

    for i in allk:
        Swi = sim3_inverse(vScw.get(i, I)) if badp.get(i, False) else I
        p = int(m.parent[i])
        if p >= 0 and p in sk:
            S = rel(i, p)
            if S is not None:
                add(i, p, sim3_mul(S, Swi))
        loops = m.loop_set(i)
        for L in sorted(loops):
            if L in sk and m.kf_id[L] < m.kf_id[i]:
                S = rel(i, L)
                if S is not None:
                    add(i, L, sim3_mul(S, Swi))
        ch = m.children(i)
        for k in m.covisibles_by_weight(i, MIN_FEAT):
            if k != p and k not in ch and k not in loops and k in sk and not m.bad[k] and m.kf_id[k] < m.kf_id[i]:
                S = rel(i, k)
                if S is not None:
                    add(i, k, sim3_mul(S, Swi))
    g = PgoGraph(est, fx, fs, np.array(edges, np.int32).reshape(-1, 2), np.array(meas).reshape(-1, 8))
    return g, kfs, vScw, vCorr, good, badp


# ---- the inertial loop of Optimizer::OptimizeEssentialGraph4DoF ----
def _quat_to_R(q):
    """Eigen's Quaternion::toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


@dataclass
class SynthInertialMap(SynthPgoMap):
    """An inertial loop map: SynthPgoMap plus mImuCalib.mTcb (float, as the keyframes keep it)."""
    Rcb: np.ndarray = None               # [3, 3] float32
    tcb: np.ndarray = None               # [3] float32

    def next_kf(self, i):
        nxt = np.flatnonzero(self.prev_kf == i)
        return int(nxt[0]) if len(nxt) else -1


def make_inertial_loop(n_kf: int, seed: int = 0, earlier_loop: bool = False, rp_noise: float = 0.0, neighbourhood: int = 4,
                       band: int = 6, id_gap: bool = True, n_points: int = 0) -> SynthInertialMap:
    """Keyframes of an IMU session on a horizontal circle (world z up), a camera mounted on the body by a Tcb that is not the
    identity, and odometry that drifts in yaw and translation only, as visual-inertial odometry does (gravity keeps roll and
    pitch).  rp_noise > 0 adds roll / pitch noise per step (radians), which the 4-DoF graph cannot remove.  The loop and its
    LoopConnections / CorrectedSim3 / NonCorrectedSim3 are laid out as in make_map."""
    rng = np.random.default_rng(seed)
    n = n_kf
    radius = max(2.0, 0.05 * n)
    theta = 2 * np.pi * np.arange(n) / n
    Rwb_t = [_rz(th + np.pi / 2) for th in theta]
    twb_t = [np.array([radius * np.cos(th), radius * np.sin(th), 0.1 * np.sin(3 * th)]) for th in theta]
    # camera: z forward along the body x, x right, y down; tilted a little and offset on the body
    Rbc = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) @ _rodrigues(np.array([0.03, -0.02, 0.05]))
    tbc = np.array([0.06, -0.02, 0.015])
    Rcb = Rbc.T.astype(np.float32)
    tcb = (-Rbc.T @ tbc).astype(np.float32)
    Rbc_f, tbc_f = Rcb.astype(np.float64).T, -Rcb.astype(np.float64).T @ tcb.astype(np.float64)
    Rd, td = [Rwb_t[0]], [twb_t[0]]
    for i in range(1, n):
        Rrel = Rwb_t[i - 1].T @ Rwb_t[i]
        trel = Rwb_t[i - 1].T @ (twb_t[i] - twb_t[i - 1])
        Rrel = Rrel @ _rz(0.5 / n + rng.normal(0, 0.002))
        if rp_noise > 0:
            Rrel = Rrel @ _rodrigues(np.array([rng.normal(0, rp_noise), rng.normal(0, rp_noise), 0.0]))
        trel = trel + rng.normal(0, 0.002, 3) + np.array([0.3 / n, 0.0, 0.0])
        Rd.append(Rd[-1] @ Rrel)
        td.append(td[-1] + Rd[-2] @ trel)
    pose_qt = np.zeros((n, 7), dtype=np.float32)
    true_qt = np.zeros((n, 7))
    for i in range(n):
        for R, t, out in ((Rd[i], td[i], pose_qt), (Rwb_t[i], twb_t[i], true_qt)):
            Rwc, twc = R @ Rbc_f, R @ tbc_f + t
            out[i, :4] = _rot_to_quat(Rwc.T)
            out[i, 4:] = -Rwc.T @ twc
    kf_id = np.array([i + i // 5 for i in range(n)] if id_gap else range(n), dtype=np.int64)
    parent = np.arange(n, dtype=np.int32) - 1
    cov = [[] for _ in range(n)]

    def connect(a, b, w):
        cov[a] = [(o, x) for o, x in cov[a] if o != b] + [(b, w)]
        cov[b] = [(o, x) for o, x in cov[b] if o != a] + [(a, w)]

    for i in range(n):
        for d in range(1, band + 1):
            if i + d < n:
                connect(i, i + d, int(260 - 30 * d + rng.integers(-10, 11)))
    cur, loop = n - 1, 1
    near_cur = list(range(n - 1, n - 1 - neighbourhood, -1))
    near_loop = list(range(0, neighbourhood + 1))
    m = SynthInertialMap(kf_id=kf_id, pose_qt=pose_qt, true_qt=true_qt, parent=parent, cov=cov, loop_edges=[],
                         prev_kf=np.arange(n, dtype=np.int32) - 1, b_imu=np.arange(n) >= 1, bad=np.zeros(n, dtype=bool),
                         mp_pos=np.zeros((0, 3), np.float32), mp_ref=np.zeros(0, np.int32), mp_corrected_by=np.zeros(0, np.int64),
                         mp_corrected_ref=np.zeros(0, np.int64), init_index=0, cur=cur, loop=loop, fix_scale=True, Rcb=Rcb, tcb=tcb)
    for a in near_cur:
        m.corrected[a] = np.concatenate([true_qt[a, :4], true_qt[a, 4:], [1.0]])
        m.noncorrected[a] = sim3_from_pose(pose_qt[a])
        conns = set()
        for b in near_loop:
            w = int(rng.integers(40, 250))
            if a == cur and b == loop:
                w = 60                      # below minFeat: kept by the (pCurKF, pLoopKF) exception
            connect(a, b, w)
            conns.add(b)
        m.connections[a] = conns
    m.connections[near_cur[1]].add(int(parent[near_cur[1]]))
    connect(near_cur[1], int(parent[near_cur[1]]), 180)
    if earlier_loop:
        m.loop_edges.append((n // 2, 2))
        m.loop_edges.append((3 * n // 4, n // 4))
        connect(n // 2, 2, 150)
    if n_points:
        m.mp_ref = rng.integers(0, n, n_points).astype(np.int32)
        pos = np.zeros((n_points, 3))
        for k, r in enumerate(m.mp_ref):
            Rwc, twc = Rd[r] @ Rbc_f, Rd[r] @ tbc_f + td[r]
            pos[k] = twc + Rwc @ np.array([rng.normal(0, 1), rng.normal(0, 0.5), 3 + rng.random() * 4])
        m.mp_pos = pos.astype(np.float32)
        m.mp_corrected_by = np.zeros(n_points, np.int64)
        m.mp_corrected_ref = np.zeros(n_points, np.int64)
    return m


def imu_pose_f32(qt, Rcb, tcb):
    """KeyFrame::GetImuRotation / GetImuPosition from a float pose: Rwb = Rwc Rcb, twb = Rwc tcb + Owc, in float."""
    f = np.float32
    Rcw = _quat_to_R(np.asarray(qt[:4], f).astype(np.float64)).astype(f)
    Rwc = Rcw.T
    Owc = (-(Rwc @ np.asarray(qt[4:], f))).astype(f)
    return (Rwc @ Rcb).astype(f), (Rwc @ tcb + Owc).astype(f)


def pack_loop4(m: SynthInertialMap, kf_pose=None):
    """src/Optimizer.cc:5300-5470 on the synthetic map: (Pgo4Graph, vertex keyframe indices, vScw by index).  Vertices are
    sorted by mnId; the edge of a bad keyframe, which the reference would dereference as a null vertex, is skipped."""
    pose = m.pose_qt if kf_pose is None else kf_pose
    Rcb, tcb = m.Rcb.astype(np.float64), m.tcb.astype(np.float64)
    vScw, entries = {}, []
    for i in range(m.n):
        if m.bad[i]:
            continue
        if i in m.corrected:
            vScw[i] = m.corrected[i]
            Swc = sim3_inverse(vScw[i])
            Rwc, twc = _quat_to_R(Swc[:4]), Swc[4:7]
            Rcw = Rwc.T
            st = (Rwc @ Rcb, Rwc @ tcb + twc, Rcw, -Rcw @ twc)
        else:
            vScw[i] = sim3_from_pose(pose[i])
            Rwb, twb = imu_pose_f32(pose[i], m.Rcb, m.tcb)
            Rcw = _quat_to_R(np.asarray(pose[i][:4], np.float32).astype(np.float64)).astype(np.float32)
            st = (Rwb.astype(np.float64), twb.astype(np.float64), Rcw.astype(np.float64),
                  np.asarray(pose[i][4:], np.float32).astype(np.float64))
        entries.append((i, st, i == m.loop))
    order = sorted(range(len(entries)), key=lambda k: m.kf_id[entries[k][0]])
    vof = {entries[k][0]: r for r, k in enumerate(order)}
    kfs = [entries[k][0] for k in order]
    sts = [entries[k][1] for k in order]
    edges, dR, dt = [], [], []

    def add(i, j, S):
        if i in vof and j in vof:
            edges.append((vof[i], vof[j]))
            dR.append(_quat_to_R(S[:4]))
            dt.append(S[4:7])

    def nc(k):
        return m.noncorrected[k] if k in m.noncorrected else vScw.get(k, np.array([0, 0, 0, 1, 0, 0, 0, 1.0]))

    inserted = set()
    for i in sorted(m.connections):
        for j in sorted(m.connections[i]):
            if (i != m.cur or j != m.loop) and m.weight(i, j) < MIN_FEAT:
                continue
            add(i, j, sim3_mul(vScw[i], sim3_inverse(vScw[j])))
            inserted.add((min(m.kf_id[i], m.kf_id[j]), max(m.kf_id[i], m.kf_id[j])))
    for i in range(m.n):
        Siw = nc(i)
        prev = int(m.prev_kf[i])
        if prev >= 0:
            add(i, prev, sim3_mul(Siw, sim3_inverse(nc(prev))))
        loops = m.loop_set(i)
        for L in sorted(loops):
            if m.kf_id[L] < m.kf_id[i]:
                add(i, L, sim3_mul(Siw, sim3_inverse(nc(L))))
        ch, nxt = m.children(i), m.next_kf(i)
        for k in m.covisibles_by_weight(i, MIN_FEAT):
            if k != prev and k != nxt and k not in ch and k not in loops and not m.bad[k] and m.kf_id[k] < m.kf_id[i]:
                if (min(m.kf_id[i], m.kf_id[k]), max(m.kf_id[i], m.kf_id[k])) in inserted:
                    continue
                add(i, k, sim3_mul(Siw, sim3_inverse(nc(k))))
    g = Pgo4Graph(np.array([s[0] for s in sts]).reshape(-1, 3, 3), np.array([s[1] for s in sts]).reshape(-1, 3),
                  np.array([s[2] for s in sts]).reshape(-1, 3, 3), np.array([s[3] for s in sts]).reshape(-1, 3),
                  np.broadcast_to(Rcb, (len(sts), 3, 3)).copy(), np.broadcast_to(tcb, (len(sts), 3)).copy(),
                  np.array([e[2] for e in (entries[k] for k in order)], bool), np.array(edges, np.int32).reshape(-1, 2),
                  np.array(dR).reshape(-1, 3, 3), np.array(dt).reshape(-1, 3), INFO_4DOF)
    return g, kfs, vScw


# ---- the stand-in map of the test-only host library ----
class HostPgoMap:
    """The synthetic map as stand-in KeyFrame / MapPoint / Map objects (osh_host_graph_create + osh_host_pgo_set_graph)."""

    def __init__(self, m: SynthPgoMap):
        self.lib = capi.load_host_library()
        self.m = m
        n, nm = m.n, len(m.mp_ref)
        f32, i32, i64 = np.float32, np.int32, np.int64
        self._keep = []

        def arr(a, dt):
            a = np.ascontiguousarray(a, dtype=dt)
            self._keep.append(a)
            return a

        kf_id, pose = arr(m.kf_id, i64), arr(m.pose_qt, f32)
        cam = arr([500, 500, 320, 240, 0], f32)
        sig = arr([1.0], f32)
        mp_id, mp_pos = arr(np.arange(nm), i64), arr(m.mp_pos.reshape(-1, 3) if nm else np.zeros((1, 3)), f32)
        P = lambda a, t: capi.ptr(a, t)  # noqa: E731
        self.g = self.lib.osh_host_graph_create(n, P(kf_id, capi.c_int64_p), P(pose, capi.c_float_p), P(cam, capi.c_float_p),
                                                P(sig, capi.c_float_p), 1, nm, P(mp_id, capi.c_int64_p), P(mp_pos, capi.c_float_p),
                                                0, None, None, None, None, int(m.kf_id[m.init_index]), 0)
        cov_kf, cov_o, cov_w = [], [], []
        for i in range(n):
            for o, w in m.cov[i]:
                cov_kf.append(i); cov_o.append(o); cov_w.append(w)  # noqa: E702
        la = [a for a, _ in m.loop_edges] or [0]
        lb = [b for _, b in m.loop_edges] or [0]
        a_cov_kf, a_cov_o, a_cov_w = arr(cov_kf or [0], i32), arr(cov_o or [0], i32), arr(cov_w or [0], i32)
        a_la, a_lb = arr(la, i32), arr(lb, i32)
        a_par, a_prev, a_imu = arr(m.parent, i32), arr(m.prev_kf, i32), arr(m.b_imu, np.uint8)
        a_ref = arr(m.mp_ref if nm else [0], i32)
        a_cb, a_cr = arr(m.mp_corrected_by if nm else [0], i64), arr(m.mp_corrected_ref if nm else [0], i64)
        rc = self.lib.osh_host_pgo_set_graph(self.g, P(a_par, capi.c_int32_p), len(cov_kf), P(a_cov_kf, capi.c_int32_p),
                                             P(a_cov_o, capi.c_int32_p), P(a_cov_w, capi.c_int32_p), len(m.loop_edges),
                                             P(a_la, capi.c_int32_p), P(a_lb, capi.c_int32_p), P(a_prev, capi.c_int32_p),
                                             P(a_imu, capi.c_uint8_p), P(a_ref, capi.c_int32_p), P(a_cb, capi.c_int64_p), P(a_cr, capi.c_int64_p))
        assert rc == 0
        for i in range(n):
            if m.bad[i]:
                self.lib.osh_host_set_bad(self.g, i, -1)
        for i, qt in m.before_merge.items():
            q = arr(qt, f32)
            self.lib.osh_host_pgo_set_before_merge(self.g, i, P(q, capi.c_float_p))

    def close(self):
        if self.g:
            self.lib.osh_host_graph_destroy(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _loop(self):
        m = self.m
        ck = list(m.corrected)
        nk = list(m.noncorrected)
        conn = [(a, b) for a in m.connections for b in m.connections[a]]
        self._lk = (np.array(ck or [0], np.int32), np.array([m.corrected[k] for k in ck] or [np.zeros(8)], np.float64).reshape(-1),
                    np.array(nk or [0], np.int32), np.array([m.noncorrected[k] for k in nk] or [np.zeros(8)], np.float64).reshape(-1),
                    np.array([a for a, _ in conn] or [0], np.int32), np.array([b for _, b in conn] or [0], np.int32))
        a, b, c, d, e, f = self._lk
        return capi.HostLoop(m.cur, m.loop, 1 if m.fix_scale else 0, len(ck), capi.ptr(a, capi.c_int32_p), capi.ptr(b, capi.c_double_p),
                             len(nk), capi.ptr(c, capi.c_int32_p), capi.ptr(d, capi.c_double_p), len(conn),
                             capi.ptr(e, capi.c_int32_p), capi.ptr(f, capi.c_int32_p))

    def _merge(self, fixed, fixed_corrected, non_fixed, mps):
        self._mk = [np.array(x or [0], np.int32) for x in (fixed, fixed_corrected, non_fixed, mps)]
        a, b, c, d = self._mk
        return capi.HostMerge(self.m.cur, len(fixed), capi.ptr(a, capi.c_int32_p), len(fixed_corrected), capi.ptr(b, capi.c_int32_p),
                              len(non_fixed), capi.ptr(c, capi.c_int32_p), len(mps), capi.ptr(d, capi.c_int32_p))

    def _out(self, max_e=None):
        n = self.m.n
        max_e = max_e or 64 * n + 64
        o = dict(kf=np.zeros(n, np.int64), est=np.zeros((n, 8)), fixed=np.zeros(n, np.uint8), fs=np.zeros(n, np.uint8),
                 eij=np.zeros((max_e, 2), np.int32), meas=np.zeros((max_e, 8)))
        st = capi.HostPgoOut(n, max_e, 0, 0, 0, capi.ptr(o["kf"], capi.c_int64_p), capi.ptr(o["est"], capi.c_double_p),
                             capi.ptr(o["fixed"], capi.c_uint8_p), capi.ptr(o["fs"], capi.c_uint8_p), capi.ptr(o["eij"], capi.c_int32_p),
                             capi.ptr(o["meas"], capi.c_double_p))
        return o, st

    def _unpack(self, o, st):
        nv, ne = st.n_vertices, st.n_edges
        g = PgoGraph(o["est"][:nv].copy(), o["fixed"][:nv].astype(bool), o["fs"][:nv].astype(bool), o["eij"][:ne].copy(), o["meas"][:ne].copy())
        return g, o["kf"][:nv].copy()

    def pack(self):
        o, st = self._out()
        assert self.lib.osh_host_pgo_pack(self.g, C.byref(self._loop()), C.byref(st)) == 0
        return self._unpack(o, st)

    def pack_merge(self, fixed, fixed_corrected, non_fixed):
        o, st = self._out()
        assert self.lib.osh_host_pgo_pack_merge(self.g, C.byref(self._merge(fixed, fixed_corrected, non_fixed, [])), C.byref(st)) == 0
        return self._unpack(o, st)

    def run(self):
        return self.lib.osh_host_pgo_run(self.g, C.byref(self._loop()))

    def run_merge(self, fixed, fixed_corrected, non_fixed, mps):
        return self.lib.osh_host_pgo_run_merge(self.g, C.byref(self._merge(fixed, fixed_corrected, non_fixed, mps)))

    def kf_poses(self):
        out = np.zeros((self.m.n, 7), np.float32)
        for i in range(self.m.n):
            self.lib.osh_host_get_kf_pose(self.g, i, capi.ptr(out[i], capi.c_float_p))
        return out

    def mp_positions(self):
        nm = len(self.m.mp_ref)
        out = np.zeros((nm, 3), np.float32)
        for j in range(nm):
            self.lib.osh_host_get_mp_pos(self.g, j, capi.ptr(out[j], capi.c_float_p))
        return out

    def normal_updates(self):
        return np.array([self.lib.osh_host_mp_normal_updates(self.g, j) for j in range(len(self.m.mp_ref))])

    def change_index(self):
        return self.lib.osh_host_map_change_index(self.g)


class HostPgo4Map(HostPgoMap):
    """An inertial map as stand-in objects: the graph of HostPgoMap plus every keyframe's mImuCalib (osh_host_graph_set_inertial
    with no preintegration), for Optimizer::OptimizeEssentialGraph4DoF (osh_host_pgo4_*)."""

    def __init__(self, m: SynthInertialMap):
        super().__init__(m)
        Rbc = m.Rcb.astype(np.float64).T
        tbc = -Rbc @ m.tcb.astype(np.float64)
        self._tbc = np.ascontiguousarray(np.concatenate([_rot_to_quat(Rbc), tbc]), dtype=np.float32)
        assert self.lib.osh_host_graph_set_inertial(self.g, 0, None, None, None, None, None, None,
                                                    capi.ptr(self._tbc, capi.c_float_p)) == 0

    def pack4(self, max_e=None):
        """The host layer's walk as (Pgo4Graph, mnId of every vertex)."""
        n = self.m.n
        max_e = max_e or 64 * n + 64
        o = dict(kf=np.zeros(n, np.int64), Rwb=np.zeros((n, 3, 3)), twb=np.zeros((n, 3)), Rcw=np.zeros((n, 3, 3)), tcw=np.zeros((n, 3)),
                 Rcb=np.zeros((n, 3, 3)), tcb=np.zeros((n, 3)), fixed=np.zeros(n, np.uint8), eij=np.zeros((max_e, 2), np.int32),
                 dR=np.zeros((max_e, 3, 3)), dt=np.zeros((max_e, 3)))
        D = lambda k: capi.ptr(o[k], capi.c_double_p)  # noqa: E731
        st = capi.HostPgo4Out(n, max_e, 0, 0, 0, capi.ptr(o["kf"], capi.c_int64_p), D("Rwb"), D("twb"), D("Rcw"), D("tcw"), D("Rcb"),
                              D("tcb"), capi.ptr(o["fixed"], capi.c_uint8_p), capi.ptr(o["eij"], capi.c_int32_p), D("dR"), D("dt"))
        assert self.lib.osh_host_pgo4_pack(self.g, C.byref(self._loop()), C.byref(st)) == 0
        nv, ne = st.n_vertices, st.n_edges
        g = Pgo4Graph(o["Rwb"][:nv].copy(), o["twb"][:nv].copy(), o["Rcw"][:nv].copy(), o["tcw"][:nv].copy(), o["Rcb"][:nv].copy(),
                      o["tcb"][:nv].copy(), o["fixed"][:nv].astype(bool), o["eij"][:ne].copy(), o["dR"][:ne].copy(), o["dt"][:ne].copy(),
                      INFO_4DOF)
        return g, o["kf"][:nv].copy()

    def run4(self):
        return self.lib.osh_host_pgo4_run(self.g, C.byref(self._loop()))
