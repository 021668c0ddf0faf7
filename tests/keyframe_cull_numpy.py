"""LocalMapping::KeyFrameCulling (src/LocalMapping.cc:932-1089) restated from its definitions, without the structure of
csrc/keyframe_cull.h: the observations of a point are a dict, a cull is a real erase (the observer deleted, its weight taken from
n_obs, the point bad at n_obs <= 2, as MapPoint::EraseObservation does), and every count starts from scratch on the map as it is.
Nothing here keeps a removed set or a state rule.

Two levels, as orb_slam3_study_kr_amd/synth_keyframe_cull.py: problems (what the device entry takes) and scenes (what the class
and the packer take)."""
from __future__ import annotations

import copy

import numpy as np

from orb_slam3_study_kr_amd.synth_keyframe_cull import CullProblem, CullScene

TH_OBS = 3


def decide(n_redundant: int, n_mps: int, th: float) -> int:
    """:1044 in float32: the product rounded to float32, then the comparison"""
    return int(np.float32(n_redundant) > np.float32(np.float32(th) * np.float32(n_mps)))


# ---------------------------------------------------------------------------------------------------------------- problems

def to_map(pb: CullProblem):
    """points: list of {'n_obs', 'bad', 'obs': {kf: (level, weight)}}; cands: list of [(point, level)]"""
    points = []
    for p in range(pb.n_points):
        e0, e1 = int(pb.point_obs_off[p]), int(pb.point_obs_off[p + 1])
        points.append({"n_obs": int(pb.point_n_obs[p]), "bad": bool(pb.point_bad[p]),
                       "obs": {int(pb.obs_kf[e]): (int(pb.obs_level[e]), int(pb.obs_weight[e])) for e in range(e0, e1)}})
    cands = [[(int(pb.slot_point[s]), int(pb.slot_level[s])) for s in range(int(pb.cand_slot_off[c]), int(pb.cand_slot_off[c + 1]))]
             for c in range(pb.n_candidates)]
    return points, cands


def erase(points, kf: int):
    """KeyFrame::SetBadFlag as far as the points see it: MapPoint::EraseObservation(kf) on every point that has the observer"""
    for p in points:
        if kf in p["obs"]:
            p["n_obs"] -= p["obs"].pop(kf)[1]
            if p["n_obs"] <= 2:
                p["bad"] = True


def count(points, slots, k: int):
    """:976-1042 for candidate k on the map as it is: (nMPs, nRedundantObservations)"""
    n_mps = n_red = 0
    for point, level in slots:
        p = points[point]
        if p["bad"]:
            continue
        n_mps += 1
        if p["n_obs"] > TH_OBS:
            n = 0
            for kf, (level_i, _w) in p["obs"].items():
                if kf == k:
                    continue
                if level_i <= level + 1:
                    n += 1
                    if n > TH_OBS:
                        break
            if n > TH_OBS:
                n_red += 1
    return n_mps, n_red


def count_under(pb: CullProblem, removed=(), first: int = 0):
    """What osh_orb_keyframe_cull_count returns: the keyframes of `removed` really erased, then every candidate from `first`"""
    points, cands = to_map(pb)
    for kf in dict.fromkeys(int(r) for r in removed):
        erase(points, kf)
    out = [count(points, cands[k], k) for k in range(first, pb.n_candidates)]
    return {"n_mps": np.array([o[0] for o in out], np.int32), "n_redundant": np.array([o[1] for o in out], np.int32),
            "redundant": np.array([decide(o[1], o[0], pb.redundant_th) for o in out], np.uint8)}


def sequential(pb: CullProblem, erasable=None, snapshot: bool = False):
    """The candidates in order: count at its turn, decide, erase when redundant (and erasable[k]).  Returns the (nMPs, nRedundant,
    decision) each candidate saw and the culled list.  snapshot: the wrong variant that never lets a cull reach the points."""
    points, cands = to_map(pb)
    seen, culled = [], []
    for k in range(pb.n_candidates):
        n_mps, n_red = count(points, cands[k], k)
        d = decide(n_red, n_mps, pb.redundant_th)
        seen.append((n_mps, n_red, d))
        if d and (erasable is None or erasable[k]):
            culled.append(k)
            if not snapshot:
                erase(points, k)
    return seen, culled


# ------------------------------------------------------------------------------------------------------------------ scenes

def scene_map(sc: CullScene):
    """Per point what MapPoint holds after the AddObservation calls of the scene: obs {kf: [left, right]}, n_obs, bad"""
    points = [{"obs": {}, "n_obs": 0, "bad": j in sc.mp_bad} for j in range(sc.n_mp)]
    for k, kf in enumerate(sc.kfs):
        for i, (p, _octave, u_right, _depth) in enumerate(kf["slots"]):
            if p < 0:
                continue
            idx = points[p]["obs"].setdefault(k, [-1, -1])
            idx[1 if (kf["n_left"] != -1 and i >= kf["n_left"]) else 0] = i
            points[p]["n_obs"] += 2 if (not kf["camera2"] and u_right >= 0) else 1
    for j, n in sc.mp_n_obs.items():
        points[j]["n_obs"] = n
    return points


def slot_level(kf, i: int) -> int:
    """scaleLevel of :1001-1003 with the right key at i - NLeft: all slots of a scene are one octave list, left keys first"""
    return kf["slots"][i][1]


def observer_level(kf, left: int, right: int) -> int:
    """scaleLeveli of :1013-1026"""
    if kf["n_left"] == -1:
        return kf["slots"][left][1]
    level = -1
    if left != -1:
        level = kf["slots"][left][1]
    if right != -1:
        r = kf["slots"][right][1]
        level = r if (level == -1 or level > r) else level
    return level


def observer_weight(kf, left: int, right: int) -> int:
    """what MapPoint::EraseObservation takes from nObs (src/MapPoint.cc:178-186)"""
    w = 0
    if left != -1:
        w += 2 if (not kf["camera2"] and kf["slots"][left][2] >= 0) else 1
    if right != -1:
        w += 1
    return w


def pack(sc: CullScene, candidates=None, monocular=None) -> dict:
    """The problem PackKeyFrameCull builds for the candidate list: the table (candidates, then observers as first met; the
    observers of a point in keyframe order, the order of the stand-in map's pointers), distinct points in slot order."""
    candidates = list(sc.covisible if candidates is None else candidates)
    monocular = sc.monocular if monocular is None else monocular
    points = scene_map(sc)
    table, table_of, first = list(candidates), {}, []
    for c, k in enumerate(candidates):
        first.append(k not in table_of)
        table_of.setdefault(k, c)
    point_of, out_points = {}, []
    off, s_point, s_level, s_index, n_obs, bad, obs_off, o_kf, o_level, o_weight = [0], [], [], [], [], [], [0], [], [], []
    for c, k in enumerate(candidates):
        kf = sc.kfs[k]
        if first[c] and kf["id"] != sc.init_kf_id and not kf["bad"]:
            for i, (p, _octave, _u, depth) in enumerate(kf["slots"]):
                if p < 0:
                    continue
                if not monocular and (np.float32(depth) > np.float32(kf["th_depth"]) or depth < 0):
                    continue
                if p not in point_of:
                    point_of[p] = len(out_points)
                    out_points.append(p)
                    n_obs.append(points[p]["n_obs"]); bad.append(int(points[p]["bad"]))
                    for ok in sorted(points[p]["obs"]):
                        left, right = points[p]["obs"][ok]
                        if ok not in table_of:
                            table_of[ok] = len(table)
                            table.append(ok)
                        o_kf.append(table_of[ok]); o_level.append(observer_level(sc.kfs[ok], left, right))
                        o_weight.append(observer_weight(sc.kfs[ok], left, right))
                    obs_off.append(len(o_kf))
                s_point.append(point_of[p]); s_level.append(slot_level(kf, i)); s_index.append(i)
        off.append(len(s_point))
    i32 = lambda a: np.asarray(a, np.int32).reshape(-1)
    return {"table_kf": i32(table), "cand_slot_off": i32(off), "slot_point": i32(s_point), "slot_level": i32(s_level), "slot_index": i32(s_index),
            "point_mp": i32(out_points), "point_n_obs": i32(n_obs), "point_bad": np.asarray(bad, np.uint8).reshape(-1), "point_obs_off": i32(obs_off),
            "obs_kf": i32(o_kf), "obs_level": i32(o_level), "obs_weight": i32(o_weight)}


def problem_of(sc: CullScene, th: float = 0.9, candidates=None, monocular=None) -> CullProblem:
    a = pack(sc, candidates, monocular)
    return CullProblem(len(a["table_kf"]), len(a["cand_slot_off"]) - 1, th, a["cand_slot_off"], a["slot_point"], a["slot_level"], a["point_n_obs"],
                       a["point_bad"], a["point_obs_off"], a["obs_kf"], a["obs_level"], a["obs_weight"])


def run_class(sc: CullScene) -> dict:
    """LocalMapping::KeyFrameCulling on a copy of the scene, statement for statement on dicts, every count from scratch.  Returns the
    culled keyframes (scene indices, list order), prev / next of every keyframe afterwards, the MergePrevious arguments
    {receiver: argument} and the points' (n_obs, bad)."""
    kfs = copy.deepcopy(sc.kfs)
    points = scene_map(sc)
    Nd = 21
    cur = kfs[sc.current]
    th = 0.9 if not sc.inertial else (0.9 if sc.monocular else 0.5)
    last_id = 0
    if sc.inertial:
        n, aux = 0, cur
        while n < Nd and aux["prev"] != -1:
            aux = kfs[aux["prev"]]
            n += 1
        last_id = aux["id"]
    culled, merged = [], {}

    def set_bad_flag(k):
        kf = kfs[k]
        if kf["id"] == sc.init_kf_id:
            return
        if kf["not_erase"]:
            return
        for p in points:
            if k in p["obs"]:
                left, right = p["obs"].pop(k)
                p["n_obs"] -= observer_weight(kf, left, right)
                if p["n_obs"] <= 2:
                    p["bad"] = True
        kf["bad"] = True
        culled.append(k)

    count_ = 0
    for k in sc.covisible:
        count_ += 1
        kf = kfs[k]
        if kf["id"] == sc.init_kf_id or kf["bad"]:
            continue
        n_mps = n_red = 0
        for i, (p, _octave, _u, depth) in enumerate(kf["slots"]):
            if p < 0 or points[p]["bad"]:
                continue
            if not sc.monocular and (np.float32(depth) > np.float32(kf["th_depth"]) or depth < 0):
                continue
            n_mps += 1
            if points[p]["n_obs"] > TH_OBS:
                level = slot_level(kf, i)
                n = sum(1 for ok, (left, right) in points[p]["obs"].items() if ok != k and observer_level(kfs[ok], left, right) <= level + 1)
                if n > TH_OBS:
                    n_red += 1
        if decide(n_red, n_mps, th):
            if sc.inertial:
                if sc.keyframes_in_map <= Nd:
                    continue
                if kf["id"] > cur["id"] - 2:
                    continue
                if kf["prev"] != -1 and kf["next"] != -1:
                    prev, nxt = kfs[kf["prev"]], kfs[kf["next"]]
                    t = np.float32(nxt["timestamp"] - prev["timestamp"])
                    d = np.asarray(kf["imu_pos"], np.float32) - np.asarray(prev["imu_pos"], np.float32)
                    near = np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) < 0.02
                    if (sc.imu_initialized and kf["id"] < last_id and t < 3.0) or t < 0.5 or (not sc.inertial_ba2 and near and t < 3):
                        merged[kf["next"]] = k
                        nxt["prev"], prev["next"] = kf["prev"], kf["next"]
                        kf["next"] = kf["prev"] = -1
                        set_bad_flag(k)
            else:
                set_bad_flag(k)
        if (count_ > 20 and sc.abort_ba) or count_ > 100:
            break
    return {"culled": culled, "prev": [kf["prev"] for kf in kfs], "next": [kf["next"] for kf in kfs], "merged": merged,
            "points": [(p["n_obs"], int(p["bad"])) for p in points]}
