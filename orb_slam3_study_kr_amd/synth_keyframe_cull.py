"""Synthetic inputs for LocalMapping::KeyFrameCulling (src/LocalMapping.cc:932-1089).

Two levels.  A ``CullProblem`` is an ``osh_kfcull_problem`` (include/orbslam3_hip.h): the records the counting kernel reads, built
directly so that every threshold of the rule can be put where a test wants it.  A ``CullScene`` is a stand-in map (keyframes with
slots, points, the covisibility list, the inertial links) for the class behind the reference signature and for the packer.

Observation lengths of ``random_problem`` and ``random_scene``: a point is seen by 2 + a geometric (p = 0.1) number of keyframes
(median 9, mean 12 over the points), and one point in 200 is a landmark seen by 65-300 keyframes.  Seen from the slots of a
keyframe the runs are longer, since a point with many observers sits in many slots: DESIGN.md section 27 gives the figures the
kernel shape is based on.
"""
from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass
class CullProblem:
    n_keyframes: int
    n_candidates: int
    redundant_th: float
    cand_slot_off: np.ndarray
    slot_point: np.ndarray
    slot_level: np.ndarray
    point_n_obs: np.ndarray
    point_bad: np.ndarray
    point_obs_off: np.ndarray
    obs_kf: np.ndarray
    obs_level: np.ndarray
    obs_weight: np.ndarray

    @property
    def n_points(self):
        return len(self.point_n_obs)


class ProblemBuilder:
    """Points with explicit observer lists, slots per candidate."""

    def __init__(self, n_keyframes: int, n_candidates: int, redundant_th: float = 0.9):
        self.n_keyframes, self.n_candidates, self.th = n_keyframes, n_candidates, redundant_th
        self.points, self.slots = [], [[] for _ in range(n_candidates)]

    def point(self, obs, n_obs=None, bad=0) -> int:
        """obs: (kf, level, weight) triples; n_obs: the point's own nObs (default: the sum of the weights)."""
        obs = [tuple(int(x) for x in o) for o in obs]
        self.points.append((sum(o[2] for o in obs) if n_obs is None else int(n_obs), int(bad), obs))
        return len(self.points) - 1

    def slot(self, cand: int, point: int, level: int = 0):
        self.slots[cand].append((point, level))

    def build(self) -> CullProblem:
        i32 = lambda a: np.asarray(a, np.int32).reshape(-1)
        off = np.cumsum([0] + [len(s) for s in self.slots])
        flat = [x for s in self.slots for x in s]
        obs_off = np.cumsum([0] + [len(p[2]) for p in self.points])
        obs = [o for p in self.points for o in p[2]]
        return CullProblem(self.n_keyframes, self.n_candidates, self.th, i32(off), i32([x[0] for x in flat]), i32([x[1] for x in flat]),
                           i32([p[0] for p in self.points]), np.asarray([p[1] for p in self.points], np.uint8).reshape(-1), i32(obs_off),
                           i32([o[0] for o in obs]), i32([o[1] for o in obs]), i32([o[2] for o in obs]))


def thresholds() -> CullProblem:
    """One candidate (table entry 0), observers 1..7.  Per point: whether the slot is redundant is in REDUNDANT_THRESHOLDS."""
    b = ProblemBuilder(8, 1)
    me = (0, 0, 1)
    cases = [
        ([me] + [(k, 0, 1) for k in (1, 2, 3)], None),            # exactly 3 other observers: no
        ([me] + [(k, 0, 1) for k in (1, 2, 3, 4)], None),         # exactly 4: yes
        ([me] + [(k, 0, 1) for k in (1, 2, 3, 4)], 3),            # 4 others but n_obs exactly 3: no
        ([me] + [(k, 0, 1) for k in (1, 2, 3, 4)], 4),            # n_obs exactly 4: yes
        ([me] + [(k, 3, 1) for k in (1, 2, 3, 4)], None),         # observer level = slot level + 1 (slot level 2): yes
        ([me] + [(k, 4, 1) for k in (1, 2, 3, 4)], None),         # level + 2: no
        ([(k, 0, 1) for k in (1, 2, 3)] + [me, (4, 3, 1)], None), # the candidate in the middle of the run, one observer too coarse: no
        ([(k, 0, 1) for k in (1, 2, 3, 4)] + [me], None),         # the candidate last in the run: yes
        ([(0, 0, 1), (1, 0, 1), (2, 0, 1), (3, 0, 1)], 9),        # the candidate counted would make 4: no
    ]
    levels = [0, 0, 0, 0, 2, 2, 0, 0, 0]
    for (obs, n_obs), lv in zip(cases, levels):
        b.slot(0, b.point(obs, n_obs), lv)
    return b.build()


REDUNDANT_THRESHOLDS = [0, 1, 0, 1, 1, 0, 0, 1, 0]


def weights() -> CullProblem:
    """Two stereo observers give n_obs = 4 > 3 with one other observer (not redundant); weights 2 and 3 leave n_obs' on either side
    of the limits when their observer is removed (REMOVED_WEIGHTS: the set, then per point (counted, redundant))."""
    b = ProblemBuilder(8, 1)
    b.slot(0, b.point([(0, 0, 2), (1, 0, 2)]))                                        # n_obs 4, one other; without 1: 2 -> bad
    b.slot(0, b.point([(0, 0, 1), (1, 0, 3), (2, 0, 1), (3, 0, 1), (4, 0, 1), (5, 0, 1)]))  # n_obs 8; without 1: 5, 4 others
    b.slot(0, b.point([(0, 0, 1), (1, 0, 3), (2, 0, 1), (3, 0, 1), (4, 0, 1), (5, 0, 1)], n_obs=6))  # without 1: 3, not > 3
    b.slot(0, b.point([(0, 0, 1), (1, 0, 2), (2, 0, 1)], n_obs=4))                    # without 1: 2 -> bad
    b.slot(0, b.point([(0, 0, 1), (1, 0, 2), (2, 0, 1)], n_obs=5))                    # without 1: 3 -> stays, not redundant
    b.slot(0, b.point([(0, 0, 1), (2, 0, 1)], n_obs=2))                               # n_obs 2 and nothing removed: not bad
    return b.build()


REMOVED_WEIGHTS = {(): [(1, 0), (1, 1), (1, 1), (1, 0), (1, 0), (1, 0)], (1,): [(0, 0), (1, 1), (1, 0), (0, 0), (1, 0), (1, 0)]}


def float_decision(n_mps: int, n_redundant: int, th: float) -> CullProblem:
    """One candidate with n_mps slots of which n_redundant are redundant."""
    b = ProblemBuilder(6, 1, th)
    for i in range(n_mps):
        others = 4 if i < n_redundant else 1
        b.slot(0, b.point([(0, 0, 1)] + [(k, 0, 1) for k in range(1, 1 + others)], n_obs=5))
    return b.build()


FLOAT_DECISIONS = [(10, 9, 0.9, 0), (10, 10, 0.9, 1), (4, 2, 0.5, 0), (4, 3, 0.5, 1), (0, 0, 0.9, 0), (0, 0, 0.5, 0)]


def random_problem(n_candidates: int, slots_per_candidate, n_keyframes: int = 400, n_points: int | None = None, seed: int = 0,
                   redundant_th: float = 0.9, long_runs=()) -> CullProblem:
    """Candidates with the given slot counts over a pool of points with the module's observation lengths; long_runs: observation
    counts of extra points placed in the first slots of candidate 0 (they need n_keyframes at least as large)."""
    rng = np.random.default_rng(seed)
    slots = [int(s) for s in (slots_per_candidate if np.ndim(slots_per_candidate) else [slots_per_candidate] * n_candidates)]
    n_points = n_points or max(8, sum(slots) // 3)
    b = ProblemBuilder(n_keyframes, n_candidates, redundant_th)
    lengths = 2 + rng.geometric(0.1, n_points)
    landmark = rng.random(n_points) < 0.005
    lengths[landmark] = rng.integers(65, 301, int(landmark.sum()))
    lengths = np.minimum(lengths, n_keyframes)
    for n in list(lengths) + list(long_runs):
        kfs = rng.choice(n_keyframes, int(n), replace=False)
        w = rng.choice([1, 1, 2, 2, 3], int(n))
        obs = [(int(k), int(rng.integers(0, 8)), int(x)) for k, x in zip(kfs, w)]
        total = int(w.sum())
        b.point(obs, n_obs=total + int(rng.integers(-1, 2)), bad=int(rng.random() < 0.03))
    for c, n in enumerate(slots):
        for i in range(n):
            p = n_points + i if (c == 0 and i < len(long_runs)) else int(rng.integers(0, n_points))
            b.slot(c, p, int(rng.integers(0, 8)))
    return b.build()


# ------------------------------------------------------------------------------------------------------------------ scenes

class CullScene:
    """A stand-in map: keyframes with slots (point, octave, uRight, depth), the current keyframe and its covisibility list."""

    def __init__(self, init_kf_id: int = 10 ** 6, keyframes_in_map: int = 100, imu_initialized: bool = False, inertial_ba2: bool = False):
        self.kfs, self.n_mp, self.mp_n_obs, self.mp_bad = [], 0, {}, set()
        self.init_kf_id, self.keyframes_in_map, self.imu_initialized, self.inertial_ba2 = init_kf_id, keyframes_in_map, imu_initialized, inertial_ba2
        self.current, self.covisible = None, []
        self.monocular, self.inertial, self.abort_ba = False, False, False

    def add_kf(self, kf_id: int, n_left: int = -1, camera2: bool = False, th_depth: float = 40.0, timestamp: float = 0.0, not_erase: bool = False,
               bad: bool = False, imu_pos=(0.0, 0.0, 0.0), preint: bool = False) -> int:
        self.kfs.append(dict(id=int(kf_id), n_left=n_left, camera2=camera2, th_depth=th_depth, timestamp=timestamp, not_erase=not_erase, bad=bad,
                             imu_pos=tuple(imu_pos), preint=preint, prev=-1, next=-1, slots=[]))
        return len(self.kfs) - 1

    def add_point(self, n_obs=None, bad: bool = False) -> int:
        self.n_mp += 1
        if n_obs is not None:
            self.mp_n_obs[self.n_mp - 1] = int(n_obs)
        if bad:
            self.mp_bad.add(self.n_mp - 1)
        return self.n_mp - 1

    def observe(self, kf: int, point: int, octave: int = 0, u_right: float = -1.0, depth: float = 1.0) -> int:
        """The next slot of the keyframe holds the point (-1: an empty slot).  Right slots of a rig come after n_left left ones."""
        self.kfs[kf]["slots"].append((int(point), int(octave), float(u_right), float(depth)))
        return len(self.kfs[kf]["slots"]) - 1

    def chain(self, kfs):
        for a, b in zip(kfs[:-1], kfs[1:]):
            self.kfs[a]["next"], self.kfs[b]["prev"] = b, a


def _observers(sc: CullScene, n: int, first_id: int = 500):
    return [sc.add_kf(first_id + i) for i in range(n)]


def _redundant_points(sc: CullScene, cand: int, others, n: int, **kw):
    """n points seen by the candidate and by `others` (4 of them make the slot redundant)."""
    pts = []
    for _ in range(n):
        p = sc.add_point()
        sc.observe(cand, p, **kw)
        for o in others:
            sc.observe(o, p)
        pts.append(p)
    return pts


def _finish(sc: CullScene, candidates, cur_id: int = 900, **flags):
    sc.current = sc.add_kf(cur_id)
    sc.covisible = list(candidates)
    for k, v in flags.items():
        setattr(sc, k, v)
    return sc


def seq_unredundant() -> CullScene:
    """A and B share 10 points seen by three more keyframes: A is redundant (4 others), and once it is gone B has exactly 3."""
    sc = CullScene()
    a, b = sc.add_kf(100), sc.add_kf(101)
    x = _observers(sc, 3)
    _redundant_points(sc, a, [b] + x, 10)
    return _finish(sc, [a, b], monocular=True)


def seq_bad_flip() -> CullScene:
    """Culling A leaves the 2 points it shares with B and one more keyframe at n_obs = 2: they go bad, B's nMPs falls from 12 to
    10 with 10 redundant, and B, not redundant before (10 > 10.8 fails), is redundant (10 > 9)."""
    sc = CullScene()
    a, b = sc.add_kf(100), sc.add_kf(101)
    x = _observers(sc, 5)
    _redundant_points(sc, a, x[:4], 30)
    _redundant_points(sc, a, [b, x[4]], 2)
    _redundant_points(sc, b, x[:4], 10)
    return _finish(sc, [a, b], monocular=True)


def seq_three_culls() -> CullScene:
    """A, B and C are redundant on 30 points of their own each (30 of 32 with the two shared ones, which stop being redundant for
    them as the others go); D's 2 points are seen by A, B, C and one more keyframe: redundant at the start, and after the three
    culls at n_obs = 2, bad, so D counts nothing."""
    sc = CullScene()
    a, b, c, d = (sc.add_kf(100 + i) for i in range(4))
    x = _observers(sc, 4)
    for k in (a, b, c):
        _redundant_points(sc, k, x, 30)
    _redundant_points(sc, d, [a, b, c, x[0]], 2)
    return _finish(sc, [a, b, c, d], monocular=True)


def seq_not_erase() -> CullScene:
    """seq_unredundant with mbNotErase on A: A is judged redundant and stays, so B still has 4 other observers and is culled."""
    sc = seq_unredundant()
    sc.kfs[sc.covisible[0]]["not_erase"] = True
    return sc


SEQUENTIAL = {"unredundant": (seq_unredundant, [100]), "bad_flip": (seq_bad_flip, [100, 101]), "three_culls": (seq_three_culls, [100, 101, 102]),
              "not_erase": (seq_not_erase, [101])}


def stereo_depth(monocular: bool) -> CullScene:
    """A candidate with 10 close redundant points and 10 far / negative-depth points that nobody else sees: with the depth test
    (stereo) it is 10 of 10 and culled, without it (monocular) 10 of 20 and kept.  Observers are stereo (weight 2)."""
    sc = CullScene()
    a = sc.add_kf(100, th_depth=35.0)
    x = _observers(sc, 4)
    _redundant_points(sc, a, x, 10, u_right=5.0, depth=35.0)
    for i in range(10):
        sc.observe(a, sc.add_point(), u_right=-1.0, depth=(35.5 if i % 2 else -1.0))
    return _finish(sc, [a], monocular=monocular)


def rig_levels() -> CullScene:
    """Rig keyframes (NLeft = 4, two right slots).  The candidate's points sit in left and right slots; observers see them with the
    left index, the right index or both, the right level lower than the left, with and without mpCamera2 (weights 1, 2 and 3)."""
    sc = CullScene()
    a = sc.add_kf(100, n_left=4, camera2=True)
    obs = [sc.add_kf(500 + i, n_left=4, camera2=(i != 1)) for i in range(5)]
    pts = [sc.add_point() for _ in range(4)]
    # candidate: points 0, 1 in left slots 0, 1 (octaves 1, 2), empty left slots, points 2, 3 in right slots 4, 5 (octaves 3, 0)
    sc.observe(a, pts[0], 1); sc.observe(a, pts[1], 2); sc.observe(a, -1); sc.observe(a, -1)
    sc.observe(a, pts[2], 3); sc.observe(a, pts[3], 0)
    for i, o in enumerate(obs):
        # left slots 0..3 hold point i % 4 at octave 4 (uRight set on keyframe 1 only, the one without mpCamera2), right slots the same
        # point at octave 2 for even i and for keyframe 1 (left with uRight and right: weight 3), the next point for i = 3
        for s in range(4):
            sc.observe(o, pts[s] if s == i % 4 else -1, 4, u_right=(3.0 if i == 1 else -1.0))
        sc.observe(o, pts[i % 4] if (i % 2 == 0 or i == 1) else pts[(i + 1) % 4], 2)
        sc.observe(o, -1)
    return _finish(sc, [a], monocular=True)


def two_slots() -> CullScene:
    """A point in two slots of one candidate (both slots count), redundant through 4 others."""
    sc = CullScene()
    a = sc.add_kf(100)
    x = _observers(sc, 4)
    p = _redundant_points(sc, a, x, 1)[0]
    sc.observe(a, p, 1)
    return _finish(sc, [a], monocular=True)


def inertial_guards(keyframes_in_map: int = 30, inertial_ba2: bool = False, monocular: bool = False) -> CullScene:
    """Inertial.  Every candidate is redundant on points of its own; the guards decide.  A temporal chain c[0..24] (ids 100..123 and
    125) ends in the current keyframe (id 126), so last_ID, 21 links back, is 104 and the id guard spares id 125.  In list order:
      c[1]   id 101 < last_ID, t = 2 < 3, IMU initialised                      -> culled, c[0] and c[2] linked
      c[2]   its mPrevKF is c[0] by then: t = 3.5 (2.5 with the old link)      -> stays
      c[10]  t = 0.4 < 0.5                                                      -> culled
      c[14]  t = 1, 0 m from its predecessor, no inertial BA2 yet               -> culled (second branch); stays with inertial_ba2
      c[18]  t = 1, 5 m from its predecessor                                    -> stays
      c[24]  id 125 > 126 - 2                                                   -> stays
      lone   no mPrevKF / mNextKF                                               -> stays
    and nothing is culled when the map has no more than 21 keyframes."""
    sc = CullScene(keyframes_in_map=keyframes_in_map, imu_initialized=True, inertial_ba2=inertial_ba2)
    x = _observers(sc, 4)
    ts = [1.5 * i for i in range(25)]
    ts[0:4] = [0.0, 1.0, 2.0, 3.5]
    ts[9:12] = [13.5, 13.7, 13.9]
    ts[13:16] = [19.5, 20.0, 20.5]
    ts[17:20] = [25.5, 26.0, 26.5]
    c = [sc.add_kf(100 + i if i < 24 else 125, timestamp=ts[i], preint=True, imu_pos=((5.0, 0.0, 0.0) if i == 18 else (0.0, 0.0, 0.0))) for i in range(25)]
    lone = sc.add_kf(90, timestamp=4.0, preint=True)
    cands = [c[1], c[2], c[10], c[14], c[18], c[24], lone]
    for k in cands:
        _redundant_points(sc, k, x, 6, u_right=5.0, depth=1.0)
    sc = _finish(sc, cands, cur_id=126, inertial=True, monocular=monocular)
    sc.kfs[sc.current].update(timestamp=40.0, preint=True)
    sc.chain(c + [sc.current])
    return sc


def ratio(inertial: bool, monocular: bool) -> CullScene:
    """One candidate with 6 redundant points of 10, between two chain neighbours 0.4 s apart: culled at redundant_th = 0.5
    (inertial stereo) and kept at 0.9 (every other mode)."""
    sc = CullScene(keyframes_in_map=30)
    x = _observers(sc, 4)
    c = [sc.add_kf(100 + i, timestamp=0.2 * i, preint=True) for i in range(3)]
    _redundant_points(sc, c[1], x, 6, u_right=5.0, depth=1.0)
    _redundant_points(sc, c[1], x[:1], 4, u_right=5.0, depth=1.0)
    sc = _finish(sc, [c[1]], cur_id=110, inertial=inertial, monocular=monocular)
    sc.kfs[sc.current].update(timestamp=5.0, preint=True)
    sc.chain(c + [sc.current])
    return sc


def count_limits(n: int, abort_ba: bool) -> CullScene:
    """n redundant candidates (independent points).  With mbAbortBA the loop leaves after the 21st, else after the 101st."""
    sc = CullScene()
    x = _observers(sc, 4)
    ks = [sc.add_kf(100 + i) for i in range(n)]
    for k in ks:
        _redundant_points(sc, k, x, 2)
    return _finish(sc, ks, cur_id=9000, monocular=True, abort_ba=abort_ba)


def skipped() -> CullScene:
    """The map's initial keyframe and an already bad keyframe in the list (both redundant by their points): skipped."""
    sc = CullScene(init_kf_id=100)
    x = _observers(sc, 4)
    ks = [sc.add_kf(100), sc.add_kf(101, bad=True), sc.add_kf(102)]
    for k in ks:
        _redundant_points(sc, k, x, 4)
    return _finish(sc, ks, monocular=True)


def big_table(n_keyframes: int) -> CullScene:
    """Two redundant candidates and n_keyframes - 2 further observers, every one of them in the table: a point of candidate 0 is
    seen by all but eight of them, and its other points by the last four.  A table of OSH_KFCULL_MAX_KEYFRAMES entries fits the
    device, one more does not."""
    sc = CullScene()
    a, b = sc.add_kf(100), sc.add_kf(101)
    x = _observers(sc, n_keyframes - 2, first_id=1000)
    _redundant_points(sc, b, x[:4], 5)
    filler = sc.add_point()
    sc.observe(a, filler)
    for o in x[4:-4]:               # puts every observer into the table, in order, through one long run
        sc.observe(o, filler)
    _redundant_points(sc, a, x[-4:], 40)
    return _finish(sc, [a, b], cur_id=9000, monocular=True)


def random_scene(n_candidates: int, slots_per_keyframe: int = 1000, n_keyframes: int = 400, seed: int = 0) -> CullScene:
    """A monocular map of n_keyframes keyframes with about slots_per_keyframe points each, the observation lengths of the module
    docstring; the first n_candidates keyframes are the covisibility list.  The workload of profiles/keyframe_cull_timing.py."""
    rng = np.random.default_rng(seed)
    sc = CullScene()
    kfs = [sc.add_kf(100 + i) for i in range(n_keyframes)]
    n_points = int(slots_per_keyframe * n_keyframes / 11.0)
    lengths = 2 + rng.geometric(0.1, n_points)
    landmark = rng.random(n_points) < 0.005
    lengths[landmark] = rng.integers(65, 301, int(landmark.sum()))
    for n in np.minimum(lengths, n_keyframes):
        p = sc.add_point()
        for k in rng.choice(n_keyframes, int(n), replace=False):
            sc.kfs[kfs[k]]["slots"].append((p, int(rng.integers(0, 8)), -1.0, 1.0))
    return _finish(sc, kfs[:n_candidates], cur_id=10 ** 5, monocular=True)
