"""Synthetic segments for the per-match body of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:503-720).

A segment is one (current keyframe, neighbour) pair with the matched keypoint pairs ORBmatcher::SearchForTriangulation would hand
over.  The camera kinds:

  mono      a pinhole keyframe pair with a sideways baseline: every pair is triangulated
  stereo    a rectified stereo pair (mb 0.1 m) whose neighbour lies 0.5 m ahead.  Close points near the image centre have less ray
            parallax than stereo parallax and take UnprojectStereo of the current keyframe, or of the neighbour when only the
            neighbour has a stereo match; points towards the image border, farther away, have more and are triangulated whether
            they carry a stereo match or not; a few beyond 40 baselines
  kb8       a monocular KannalaBrandt8 pair
  rig       a KannalaBrandt8 stereo rig (NLeft != -1, mpCamera2): the four left / right combinations in one segment
  w_zero    keyframes whose Rwc is not the transpose of Rcw and keypoints on the principal point: the third column of A is exactly
            zero and so is the fourth entry of its null vector (x3Dh(3) == 0); the rays still have parallax because Rwc says so.
            The entry takes the four arrays of a pose as given
  zero_dist identical stereo pairs of the neighbour whose point is exactly the current keyframe's Ow (an Ow that does not belong
            to its pose): dist1 == 0

Every true pair gets pixel noise growing with its octave and octaves that follow the distance ratio.  Outlier groups, drawn per
pair: wrong (the second keypoint belongs to another point), scale (octaves seven levels apart), reproj2 (the second keypoint
9 px off the epipolar line, a coarse first octave and a fine second one: only the neighbour's test fails), no_depth (mvuRight >= 0
with mvDepth 0), behind2 (stereo of the current keyframe: a depth the neighbour has already passed), low (points 100 m away:
parallax below either limit; few, because every cosine from 0.9988 up lies within the restatement's relative 1e-3 of 0.9996 /
0.9998 and counts as borderline).  With far_points the limit th_far cuts the true points about in half.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import synth_fisheye as sf

F = np.float32
PINHOLE, KB8 = 0, 1
N_LEVELS = 8
PIN = np.array([458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0], F)   # public EuRoC cam0 intrinsics
WIDTH, HEIGHT = 752, 480
MB = 0.1
RIG_ROTVEC, RIG_T = (0.010, -0.020, 0.005), (-0.1, 0.002, 0.01)     # the rig's mTrl: x_right = R x_left + t


@dataclasses.dataclass
class Camera:
    type: int
    params: np.ndarray      # [8] float32
    precision: float = 1e-6


@dataclasses.dataclass
class Pose:
    Rcw: np.ndarray         # [3, 3] float32
    tcw: np.ndarray
    Rwc: np.ndarray
    Ow: np.ndarray


@dataclasses.dataclass
class KeyFrame:
    pose: Pose
    camera: Camera
    right_pose: Pose | None = None
    camera2: Camera | None = None
    fx: float = 0.0
    fy: float = 0.0
    cx: float = 0.0
    cy: float = 0.0
    invfx: float = 0.0
    invfy: float = 0.0
    mbf: float = 0.0
    mb: float = 0.0
    n_left: int = -1
    n_keys: int = 0
    level_sigma2: np.ndarray = None
    scale_factors: np.ndarray = None


@dataclasses.dataclass
class Segment:
    kf1: KeyFrame
    kf2: KeyFrame
    ratio_factor: float
    inertial: bool
    far_points: bool
    th_far_points: float
    idx1: np.ndarray        # [n] int32
    idx2: np.ndarray
    pt1: np.ndarray         # [n, 2] float32
    pt2: np.ndarray
    octave1: np.ndarray     # [n] int32
    octave2: np.ndarray
    u_right1: np.ndarray    # [n] float32
    u_right2: np.ndarray
    depth1: np.ndarray
    depth2: np.ndarray
    kind: np.ndarray = None     # [n] the group every pair was built as (a census aid, not an input)
    name: str = ""
    world: np.ndarray = None    # [n, 3] the point the first keypoint was made from (a census aid, not an input)

    @property
    def n(self) -> int:
        return int(self.idx1.shape[0])

    def head(self, n: int) -> "Segment":
        """The first n matches."""
        cut = {f: getattr(self, f)[:n] for f in ("idx1", "idx2", "pt1", "pt2", "octave1", "octave2", "u_right1", "u_right2", "depth1", "depth2", "kind")
               if getattr(self, f) is not None}
        if self.world is not None:
            cut["world"] = self.world[:n]
        return dataclasses.replace(self, **cut)


def scale_factors(n_levels: int = N_LEVELS) -> np.ndarray:
    s = np.ones(n_levels, F)
    for i in range(1, n_levels):
        s[i] = F(s[i - 1] * F(sf.SCALE))
    return s


def make_pose(R, t) -> Pose:
    """Tcw = [R | t] rounded to float32, Rwc its transpose, Ow = -Rwc tcw in float32."""
    Rcw = np.asarray(R, np.float64).astype(F)
    tcw = np.asarray(t, np.float64).astype(F)
    Rwc = np.ascontiguousarray(Rcw.T)
    return Pose(Rcw, tcw, Rwc, (-(Rwc @ tcw)).astype(F))


def _keyframe(pose, camera, n_keys, right_pose=None, camera2=None, n_left=-1, mb=0.0) -> KeyFrame:
    p = camera.params
    s = scale_factors()
    return KeyFrame(pose=pose, camera=camera, right_pose=right_pose, camera2=camera2, fx=float(p[0]), fy=float(p[1]), cx=float(p[2]),
                    cy=float(p[3]), invfx=float(F(1) / p[0]), invfy=float(F(1) / p[1]), mbf=float(F(mb) * p[0]), mb=float(F(mb)),
                    n_left=n_left, n_keys=n_keys, level_sigma2=(s * s).astype(F), scale_factors=s)


def project(cam: Camera, X) -> np.ndarray:
    """Float64 projection of a camera-frame point."""
    if cam.type == KB8:
        return sf.project(cam.params, X)
    p = cam.params.astype(np.float64)
    return np.array([p[0] * X[0] / X[2] + p[2], p[1] * X[1] / X[2] + p[3]])


def _unproject_dir(cam: Camera, uv) -> np.ndarray:
    """A unit direction through pixel uv (KB8: the undistorted angle is taken for the distorted one, close enough to place a point)."""
    p = cam.params.astype(np.float64)
    x, y = (uv[0] - p[2]) / p[0], (uv[1] - p[3]) / p[1]
    if cam.type == KB8:
        th = math.hypot(x, y)
        d = np.array([math.sin(th) * x / max(th, 1e-12), math.sin(th) * y / max(th, 1e-12), math.cos(th)])
    else:
        d = np.array([x, y, 1.0])
    return d / np.linalg.norm(d)


def _to_cam(pose: Pose, X) -> np.ndarray:
    return pose.Rcw.astype(np.float64) @ X + pose.tcw.astype(np.float64)


def _to_world(pose: Pose, Xc) -> np.ndarray:
    return pose.Rwc.astype(np.float64) @ (Xc - pose.tcw.astype(np.float64))


def make_segment(seed: int, kind: str = "mono", n: int = 300, inertial: bool = False, far_points: bool = False, th_far: float = 3.0,
                 outliers: float = 0.30, low: float = 0.008, scene: dict | None = None) -> Segment:
    """One segment of `n` matches of camera kind mono / stereo / kb8 / rig; `outliers`: the share of the outlier groups together,
    `low`: the share of low-parallax pairs.  scene (make_scene): the segment of one more neighbour of a current keyframe that exists
    already -- `current` its first segment, `t21` where the neighbour stands, `reuse` matches of earlier segments whose feature of
    the current keyframe this neighbour sees too, `free1` the features of the current keyframe not used so far; every feature of
    either keyframe then appears in one match at most."""
    if kind == "w_zero":
        return _w_zero_segment(n)
    if kind == "zero_dist":
        return _zero_dist_segment(n)
    rng = np.random.default_rng(seed)
    stereo, rig = kind == "stereo", kind == "rig"
    n_keys = 1000
    cam = Camera(KB8, sf.CAM1.copy()) if kind in ("kb8", "rig") else Camera(PINHOLE, PIN.copy())
    cam_r = Camera(KB8, sf.CAM2.copy()) if rig else None
    R1 = sf.rotation(rng.normal(size=3) * 0.2)
    t1 = rng.normal(size=3) * 2.0
    pose1 = make_pose(R1, t1) if scene is None else scene["current"].kf1.pose
    # the neighbour in the current keyframe's frame: X2 = R21 X1 + t21
    if stereo:
        R21, t21 = sf.rotation(rng.normal(size=3) * 0.01), np.array([0.01, -0.01, -0.5])      # 0.5 m ahead
    else:
        R21, t21 = sf.rotation(rng.normal(size=3) * 0.05), np.array([-0.4, 0.03, -0.06])      # 0.4 m to the right
    if scene is not None and scene.get("t21") is not None:
        t21 = np.asarray(scene["t21"], np.float64)
    pose2 = make_pose(R21 @ pose1.Rcw.astype(np.float64), R21 @ pose1.tcw.astype(np.float64) + t21)
    pose1r = pose2r = None
    n_left = -1
    if rig:
        Rrl, trl = sf.rotation(RIG_ROTVEC), np.array(RIG_T)
        pose1r = make_pose(Rrl @ pose1.Rcw.astype(np.float64), Rrl @ pose1.tcw.astype(np.float64) + trl)
        pose2r = make_pose(Rrl @ pose2.Rcw.astype(np.float64), Rrl @ pose2.tcw.astype(np.float64) + trl)
        n_left = 600
    kf1 = _keyframe(pose1, cam, n_keys, pose1r, cam_r, n_left, MB if stereo else 0.0)
    kf2 = _keyframe(pose2, cam, n_keys, pose2r, cam_r, n_left, MB if stereo else 0.0)
    sc = kf1.scale_factors.astype(np.float64)
    width, height = (WIDTH, HEIGHT) if cam.type == PINHOLE else (sf.IMG, sf.IMG)

    groups = ["wrong", "scale", "reproj2"] * 2 + (["no_depth", "behind2"] if stereo else [])
    seg = dict(idx1=[], idx2=[], pt1=[], pt2=[], octave1=[], octave2=[], u_right1=[], u_right2=[], depth1=[], depth2=[], kind=[], world=[])
    true_points = []
    reuse = list(scene["reuse"]) if scene is not None else []
    next2 = [0, n_left]                      # scene: the neighbour's features are handed out in turn, left and right
    for i in range(n):
        u = rng.random()
        g = groups[int(rng.integers(len(groups)))] if u < outliers else "low" if u < outliers + low else "true"
        right1 = right2 = False
        if rig:
            right1, right2 = bool(rng.integers(2)), bool(rng.integers(2))
        old = reuse[i] if i < len(reuse) else None
        if old is not None:
            g, right1 = "true", bool(old["right1"])
        P1, P2 = (pose1r if right1 else pose1), (pose2r if right2 else pose2)
        C1, C2 = (cam_r if right1 else cam), (cam_r if right2 else cam)
        # a point in the frame of the first camera
        central = stereo and g in ("true", "no_depth", "behind2") and rng.random() < 0.45
        far = stereo and not central and rng.random() < 0.015
        if old is not None:
            central = bool(old["central"])
            X = old["world"]
            Xc1, Xc2 = _to_cam(P1, X), _to_cam(P2, X)
            uv2 = project(C2, Xc2)
        while old is None:
            if stereo and central:
                uv = np.array([cam.params[2] + rng.uniform(-20, 20), cam.params[3] + rng.uniform(-20, 20)])
                d = rng.uniform(1.0, 1.4)
            elif stereo:
                uv = np.array([cam.params[2] + rng.choice([-1, 1]) * rng.uniform(210, 350), cam.params[3] + rng.uniform(-200, 200)])
                d = rng.uniform(4.5, 6.0) if far else rng.uniform(1.5, 3.0)
            else:
                lo, hi = (0.1, 0.9) if cam.type == PINHOLE else (0.25, 0.75)      # a fisheye sees along the baseline, where parallax ends
                uv = np.array([rng.uniform(lo, hi) * width, rng.uniform(lo, hi) * height])
                d = rng.uniform(1.5, 5.0 if cam.type == PINHOLE else 4.0)
            if g == "low":
                d = 100.0
            Xc1 = _unproject_dir(C1, uv) * d
            X = _to_world(P1, Xc1)
            Xc2 = _to_cam(P2, X)
            if Xc2[2] <= 0.2:
                continue
            uv2 = project(C2, Xc2)
            if 5 <= uv2[0] < width - 5 and 5 <= uv2[1] < height - 5:
                break
        d1, d2 = np.linalg.norm(Xc1), np.linalg.norm(Xc2)
        o1 = int(rng.integers(1, 5)) if old is None else int(old["o1"])
        o2 = int(np.clip(o1 - round(math.log(d2 / d1) / math.log(sf.SCALE)), 0, N_LEVELS - 1))
        p1 = project(C1, Xc1) + rng.normal(size=2) * 0.4 * sc[o1]
        p2 = uv2 + rng.normal(size=2) * 0.4 * sc[o2]
        ur1 = ur2 = dep1 = dep2 = -1.0
        if stereo:
            # which keyframe has a stereo match for the keypoint: the close central points need one
            has1, has2 = (rng.random() < 0.5, True) if central else (rng.random() < 0.5, rng.random() < 0.5)
            if g == "behind2":
                has1 = True
            if has1:
                ur1 = p1[0] - kf1.mbf / Xc1[2] + rng.normal() * 0.3 * sc[o1]
                dep1 = kf1.mbf / (p1[0] - ur1)
            if has2:
                ur2 = p2[0] - kf2.mbf / Xc2[2] + rng.normal() * 0.3 * sc[o2]
                dep2 = kf2.mbf / (p2[0] - ur2)
        if old is not None:
            p1, ur1, dep1 = np.asarray(old["p1"], np.float64), float(old["ur1"]), float(old["dep1"])
        if g == "wrong" and true_points:
            other = true_points[int(rng.integers(len(true_points)))]
            p2 = project(C2, _to_cam(P2, other)) + rng.normal(size=2)
            if not (0 <= p2[0] < width and 0 <= p2[1] < height):
                p2 = np.array([rng.uniform(0, width), rng.uniform(0, height)])
        elif g == "scale":
            o1, o2 = (0, 7) if rng.random() < 0.5 else (7, 0)
        elif g == "reproj2":
            # a coarse first octave forgives what the fine second one does not
            o1, o2 = 6, 0
            turn = rng.uniform(0, 2 * math.pi) if stereo else math.pi / 2 * rng.choice([-1, 1])
            p2 = p2 + 9.0 * np.array([math.cos(turn), math.sin(turn)])
        elif g == "no_depth":
            ur1, dep1 = (p1[0] - 5.0, 0.0)
        elif g == "behind2":
            dep1 = rng.uniform(0.2, 0.4)           # the neighbour is 0.5 m ahead
            ur1 = p1[0] - kf1.mbf / dep1
        if g == "true":
            true_points.append(X)
        base1, base2 = (n_left if right1 else 0), (n_left if right2 else 0)
        span = (n_keys - n_left) if rig else n_keys
        if scene is None:
            seg["idx1"].append(base1 + int(rng.integers(n_left if rig and not right1 else span)))
            seg["idx2"].append(base2 + int(rng.integers(n_left if rig and not right2 else span)))
        else:
            seg["idx1"].append(int(old["idx1"]) if old is not None else scene["free1"][int(right1)].pop())
            seg["idx2"].append(next2[int(right2)])
            next2[int(right2)] += 1
        seg["world"].append(X)
        seg["pt1"].append(p1); seg["pt2"].append(p2); seg["octave1"].append(o1); seg["octave2"].append(o2)
        seg["u_right1"].append(ur1); seg["u_right2"].append(ur2); seg["depth1"].append(dep1); seg["depth2"].append(dep2)
        seg["kind"].append(g + ("/central" if central else ""))
    i32 = lambda k: np.asarray(seg[k], np.int32).reshape(n)
    f32 = lambda k, *shape: np.ascontiguousarray(np.asarray(seg[k], np.float64).astype(F).reshape(n, *shape))
    return Segment(kf1=kf1, kf2=kf2, ratio_factor=float(F(1.5) * F(sf.SCALE)), inertial=inertial, far_points=far_points,
                   th_far_points=float(F(th_far)), idx1=i32("idx1"), idx2=i32("idx2"), pt1=f32("pt1", 2), pt2=f32("pt2", 2),
                   octave1=i32("octave1"), octave2=i32("octave2"), u_right1=f32("u_right1"), u_right2=f32("u_right2"),
                   depth1=f32("depth1"), depth2=f32("depth2"), kind=np.asarray(seg["kind"]), name=f"{kind}{seed}",
                   world=np.asarray(seg["world"], np.float64).reshape(n, 3))


def _flat_segment(kf1, kf2, n, pt1, pt2, ur2=-1.0, dep2=-1.0, name="") -> Segment:
    rep = lambda v, *shape: np.ascontiguousarray(np.broadcast_to(np.asarray(v, F), (n, *shape)))
    idx = np.arange(n, dtype=np.int32)
    zero = np.zeros(n, np.int32)
    return Segment(kf1=kf1, kf2=kf2, ratio_factor=float(F(1.5) * F(sf.SCALE)), inertial=False, far_points=False, th_far_points=0.0,
                   idx1=idx, idx2=idx.copy(), pt1=rep(pt1, 2), pt2=rep(pt2, 2), octave1=zero, octave2=zero.copy(),
                   u_right1=rep(-1.0), u_right2=rep(ur2), depth1=rep(-1.0), depth2=rep(dep2), kind=np.asarray([name] * n), name=name)


def _w_zero_segment(n: int) -> Segment:
    cam = Camera(PINHOLE, PIN.copy())
    eye = np.eye(3, dtype=F)
    p1 = Pose(eye.copy(), np.array([0.3, 0.2, 0.0], F), eye.copy(), np.array([-0.3, -0.2, 0.0], F))
    turned = sf.rotation((0.0, 0.2, 0.0)).astype(F)     # the rays are 0.2 rad apart although both Rcw are the identity
    p2 = Pose(eye.copy(), np.array([-0.4, -0.1, 0.0], F), turned, np.array([0.4, 0.1, 0.0], F))
    centre = (PIN[2], PIN[3])
    return _flat_segment(_keyframe(p1, cam, n), _keyframe(p2, cam, n), n, centre, centre, name="w_zero")


def _zero_dist_segment(n: int) -> Segment:
    """The neighbour at the origin looks along z at a stereo point 2 m ahead; the current keyframe, 1 cm to the side, sees it in its
    own pixel but claims the point itself as its camera centre."""
    cam = Camera(PINHOLE, PIN.copy())
    eye = np.eye(3, dtype=F)
    depth = F(2.0)
    p2 = Pose(eye.copy(), np.zeros(3, F), eye.copy(), np.zeros(3, F))
    p1 = Pose(eye.copy(), np.array([0.01, 0.0, 0.0], F), eye.copy(), np.array([0.0, 0.0, depth], F))
    kf1, kf2 = _keyframe(p1, cam, n, mb=MB), _keyframe(p2, cam, n, mb=MB)
    u1 = F(F(F(PIN[0] * F(0.01)) / depth) + PIN[2])
    ur2 = F(PIN[2] - F(F(kf1.mbf) * F(1.0 / float(depth))))
    return _flat_segment(kf1, kf2, n, (u1, PIN[3]), (PIN[2], PIN[3]), ur2=ur2, dep2=depth, name="zero_dist")


@dataclasses.dataclass
class Scene:
    """A current keyframe and its neighbours for LocalMapping::CreateNewMapPoints: segments[k] holds the pairs SearchForTriangulation
    finds between the current keyframe (segments[k].kf1, the same in all) and neighbour k, in ascending idx1; every feature of a
    neighbour appears in one pair at most, a feature of the current keyframe in one pair per neighbour at most."""
    kind: str
    segments: list
    monocular: bool
    inertial: bool
    far_points: bool
    th_far_points: float
    map_points: list            # per neighbour: (features that hold a map point already [m], their positions [m, 3])


def make_scene(seed: int, kind: str, n: int = 120, shared: int = 25, inertial: bool = True, far_points: bool = False, th_far: float = 3.2) -> Scene:
    """Three neighbours: two a proper baseline away, the second seeing `shared` of the features the first one matched, and a third
    that fails the baseline test (2 cm away; the rig keyframes have mb = 0.2 here, every neighbour 40 map points about 3 m ahead
    for the monocular median depth).  The outlier groups of make_segment are all there, so the scene is one for the coarse search
    (mbInertial, RECENTLY_LOST, GetIniertialBA2), which does not ask for the epipolar constraint."""
    stereo, rig = kind == "stereo", kind == "rig"
    kw = dict(kind=kind, n=n, inertial=inertial, far_points=far_points, th_far=th_far)
    first = make_segment(seed, **kw)
    # make_segment draws idx1 at random: hand the first segment distinct features too
    n_keys, n_left = first.kf1.n_keys, first.kf1.n_left
    rng = np.random.default_rng(seed + 1000)
    pool = [list(rng.permutation(n_left if rig else n_keys)), list(rng.permutation(np.arange(n_left, n_keys))) if rig else []]
    first_right = (first.idx1 >= n_left) if rig else np.zeros(first.n, bool)
    first.idx1 = np.array([pool[int(r)].pop() for r in first_right], np.int32)
    count2 = [0, n_left]
    idx2 = []
    for r in ((first.idx2 >= n_left) if rig else np.zeros(first.n, bool)):
        idx2.append(count2[int(r)]); count2[int(r)] += 1
    first.idx2 = np.array(idx2, np.int32)
    segments = [first]
    true = [j for j in range(first.n) if str(first.kind[j]).startswith("true")][:shared]
    reuse = [dict(idx1=first.idx1[j], world=first.world[j], p1=first.pt1[j], o1=first.octave1[j], ur1=first.u_right1[j], dep1=first.depth1[j],
                  right1=bool(first_right[j]), central=str(first.kind[j]).endswith("central")) for j in true]
    places = [np.array([0.01, 0.01, -0.45]) if stereo else np.array([0.35, -0.02, 0.05]), np.array([0.0, 0.0, -0.02]) if stereo else np.array([-0.02, 0.0, 0.0])]
    for k, t21 in enumerate(places):
        segments.append(make_segment(seed + 1 + k, scene=dict(current=first, t21=t21, reuse=reuse if k == 0 else [], free1=pool), **kw))
    for k, sg in enumerate(segments):
        order = np.argsort(sg.idx1, kind="stable")
        for f in ("idx1", "idx2", "pt1", "pt2", "octave1", "octave2", "u_right1", "u_right2", "depth1", "depth2", "kind", "world"):
            setattr(sg, f, np.ascontiguousarray(getattr(sg, f)[order]))
        sg.kf1 = first.kf1
        if stereo or rig:
            sg.kf2 = dataclasses.replace(sg.kf2, mb=0.2 if rig else sg.kf2.mb)
    if rig:
        first.kf1.mb = 0.2
    map_points = []
    for sg in segments:
        used = set(int(i) for i in sg.idx2)
        feats = np.array([i for i in range(n_keys - 1, -1, -1) if i not in used][:40], np.int32)
        depth = np.random.default_rng(seed + 7).uniform(2.5, 3.5, feats.size)
        pos = np.array([_to_world(sg.kf2.pose, np.array([0.1, -0.1, d])) for d in depth]).reshape(-1, 3).astype(F)
        map_points.append((feats, pos))
    return Scene(kind=kind, segments=segments, monocular=kind in ("mono", "kb8"), inertial=inertial, far_points=far_points,
                 th_far_points=float(F(th_far)), map_points=map_points)
