"""ctypes driver of the C++ host layer (include/orbslam3_hip_host.h): builds the reference's pointer graph
(KeyFrame / MapPoint / Map, Frame) from flat arrays and calls ORB_SLAM3::Optimizer::LocalBundleAdjustment /
ORB_SLAM3::ORBmatcher::SearchByProjection through their own C++ signatures."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, synth
from .synth import LbaWindow


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class HostGraph:
    """A map built from a synthetic LbaWindow: keyframe k <-> pose index k of the window, point j <-> point j.

    Keyframe ids: optimisable poses get ids 100+i (ascending with the pose index, so the Hessian order of the
    reference equals the window's order), fixed poses get ids 10+i (older keyframes).  The current keyframe is
    the newest optimisable one; every other optimisable keyframe is covisible with it."""

    def __init__(self, w: LbaWindow, init_kf_fixed: bool = False, inertial: bool = False, init_kf_id_index: int | None = None):
        self.lib = capi.load_host_library()
        self.w = w
        P, F = w.n_free, w.n_fixed
        self.kf_id = np.array([100 + i for i in range(P)] + [10 + i for i in range(F)], dtype=np.int64)
        self.mp_id = np.arange(w.n_points, dtype=np.int64) + 1000
        pose = _f32(w.pose_qt)
        cam5 = _f32(w.pose_cam[0])
        inv = _f32(synth.INV_LEVEL_SIGMA2)
        # a fisheye rig window: OSH_EDGE_BODY edges are right-camera observations, added after the left ones (set_rig below)
        body = w.edge_kind == capi.OSH_EDGE_BODY
        left = ~body
        all_octave = _i32(np.round(np.log(1.0 / w.edge_info) / np.log(1.44)).astype(np.int32))
        octave = _i32(all_octave[left])
        obs = _f32(w.edge_obs[left])
        obs[w.edge_kind[left] == capi.OSH_EDGE_MONO, 2] = -1.0
        init_id = int(self.kf_id[0]) if init_kf_fixed else -1 & 0x7FFFFFFF
        if init_kf_id_index is not None:      # the map's initial keyframe (Map::GetInitKFid / GetOriginKF) is keyframe number ...
            init_id = int(self.kf_id[init_kf_id_index])
        self.init_kf_fixed = init_kf_fixed
        mp_pos = _f32(w.points)
        self._keep = [pose, cam5, inv, octave, obs, mp_pos]
        self.g = C.c_void_p(self.lib.osh_host_graph_create(
            P + F, capi.ptr(self.kf_id, capi.c_int64_p), capi.ptr(pose, capi.c_float_p), capi.ptr(cam5, capi.c_float_p),
            capi.ptr(inv, capi.c_float_p), len(inv), w.n_points, capi.ptr(self.mp_id, capi.c_int64_p),
            capi.ptr(mp_pos, capi.c_float_p), int(left.sum()), capi.ptr(_i32(w.edge_pose[left]), capi.c_int32_p),
            capi.ptr(_i32(w.edge_point[left]), capi.c_int32_p), capi.ptr(obs, capi.c_float_p), capi.ptr(octave, capi.c_int32_p),
            init_id, int(inertial)))
        if w.kb8 is not None:     # monocular fisheye map: every keyframe's mpCamera is one KannalaBrandt8
            self.lib.osh_host_graph_set_fisheye(self.g, capi.ptr(_f32(w.kb8), capi.c_float_p))
        if w.cam2 is not None:    # fisheye stereo rig: right camera, Trl and the right-camera observations
            r_uv = _f32(w.edge_obs[body][:, :2])
            rc = self.lib.osh_host_graph_set_rig(self.g, capi.ptr(_f32(w.cam2), capi.c_float_p), capi.ptr(_f32(w.trl), capi.c_float_p),
                                                 int(body.sum()), capi.ptr(_i32(w.edge_pose[body]), capi.c_int32_p),
                                                 capi.ptr(_i32(w.edge_point[body]), capi.c_int32_p), capi.ptr(r_uv, capi.c_float_p),
                                                 capi.ptr(_i32(all_octave[body]), capi.c_int32_p))
            assert rc == 0
        self.cur = P - 1
        cov = _i32([i for i in range(P) if i != self.cur])
        self.lib.osh_host_graph_set_covisible(self.g, self.cur, len(cov), capi.ptr(cov, capi.c_int32_p))

    def close(self):
        if self.g:
            self.lib.osh_host_graph_destroy(self.g)
            self.g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def pack(self):
        sizes = np.zeros(5, dtype=np.int32)
        null = [None] * 10
        rc = self.lib.osh_host_pack_lba(self.g, self.cur, capi.ptr(sizes, capi.c_int32_p), *[C.cast(None, t) for t in (
            capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_int32_p, capi.c_int32_p, capi.c_uint8_p, capi.c_double_p,
            capi.c_double_p, capi.c_int64_p, capi.c_int64_p)])
        del null
        if rc != 0:
            return rc, sizes, None
        P, F, L, E = (int(x) for x in sizes[:4])
        out = dict(pose_qt=np.zeros((P + F, 7)), pose_cam=np.zeros((P + F, 5)), points=np.zeros((L, 3)),
                   edge_pose=np.zeros(E, dtype=np.int32), edge_point=np.zeros(E, dtype=np.int32), edge_kind=np.zeros(E, dtype=np.uint8),
                   edge_obs=np.zeros((E, 3)), edge_info=np.zeros(E), pose_kf_id=np.zeros(P + F, dtype=np.int64),
                   point_mp_id=np.zeros(L, dtype=np.int64))
        d, i32, u8, i64 = capi.c_double_p, capi.c_int32_p, capi.c_uint8_p, capi.c_int64_p
        rc = self.lib.osh_host_pack_lba(self.g, self.cur, capi.ptr(sizes, i32), capi.ptr(out["pose_qt"], d), capi.ptr(out["pose_cam"], d),
                                        capi.ptr(out["points"], d), capi.ptr(out["edge_pose"], i32), capi.ptr(out["edge_point"], i32),
                                        capi.ptr(out["edge_kind"], u8), capi.ptr(out["edge_obs"], d), capi.ptr(out["edge_info"], d),
                                        capi.ptr(out["pose_kf_id"], i64), capi.ptr(out["point_mp_id"], i64))
        return rc, sizes, out

    def packed_window(self) -> LbaWindow:
        """The osh_lba_problem the host layer builds for the current keyframe, as an LbaWindow (for the oracle)."""
        rc, sizes, o = self.pack()
        assert rc == 0, rc
        return LbaWindow(n_free=int(sizes[0]), n_fixed=int(sizes[1]), pose_qt=o["pose_qt"], pose_cam=o["pose_cam"], points=o["points"],
                         edge_pose=o["edge_pose"], edge_point=o["edge_point"], edge_kind=o["edge_kind"], edge_obs=o["edge_obs"],
                         edge_info=o["edge_info"], lambda_init=0.0, max_iterations=10, kb8=self._last_kb8(),
                         cam2=self._last_rig()[0], trl=self._last_rig()[1]).normalise(), o

    def _last_rig(self):
        c, t = np.zeros(8), np.zeros(7)
        return (c, t) if self.lib.osh_host_last_pack_rig(self.g, capi.ptr(c, capi.c_double_p), capi.ptr(t, capi.c_double_p)) else (None, None)

    def _last_kb8(self):
        k = np.zeros(4)
        return k if self.lib.osh_host_last_pack_kb8(self.g, capi.ptr(k, capi.c_double_p)) else None

    def run_lba(self, stop_flag: np.ndarray | None = None):
        counts = np.zeros(4, dtype=np.int32)
        rc = self.lib.osh_host_run_lba(self.g, self.cur, capi.ptr(stop_flag, capi.c_uint8_p) if stop_flag is not None else
                                       C.cast(None, capi.c_uint8_p), capi.ptr(counts, capi.c_int32_p))
        assert rc == 0
        return counts

    # ---- Optimizer::GlobalBundleAdjustemnt
    def packed_global_window(self, max_iterations=5, robust=True):
        """The osh_lba_problem the host layer builds for BundleAdjustment over the whole graph, as an LbaWindow."""
        sizes = np.zeros(5, dtype=np.int32)
        d, i32, u8, i64 = capi.c_double_p, capi.c_int32_p, capi.c_uint8_p, capi.c_int64_p
        rc = self.lib.osh_host_pack_gba(self.g, capi.ptr(sizes, i32), *[C.cast(None, t) for t in (d, d, d, i32, i32, u8, d, d, i64, i64)])
        assert rc == 0, rc
        P, F, L, E = (int(x) for x in sizes[:4])
        o = dict(pose_qt=np.zeros((P + F, 7)), pose_cam=np.zeros((P + F, 5)), points=np.zeros((L, 3)),
                 edge_pose=np.zeros(E, dtype=np.int32), edge_point=np.zeros(E, dtype=np.int32), edge_kind=np.zeros(E, dtype=np.uint8),
                 edge_obs=np.zeros((E, 3)), edge_info=np.zeros(E), pose_kf_id=np.zeros(P + F, dtype=np.int64),
                 point_mp_id=np.zeros(L, dtype=np.int64), n_not_included=int(sizes[4]))
        rc = self.lib.osh_host_pack_gba(self.g, capi.ptr(sizes, i32), capi.ptr(o["pose_qt"], d), capi.ptr(o["pose_cam"], d),
                                        capi.ptr(o["points"], d), capi.ptr(o["edge_pose"], i32), capi.ptr(o["edge_point"], i32),
                                        capi.ptr(o["edge_kind"], u8), capi.ptr(o["edge_obs"], d), capi.ptr(o["edge_info"], d),
                                        capi.ptr(o["pose_kf_id"], i64), capi.ptr(o["point_mp_id"], i64))
        assert rc == 0, rc
        w = LbaWindow(n_free=P, n_fixed=F, pose_qt=o["pose_qt"], pose_cam=o["pose_cam"], points=o["points"],
                      edge_pose=o["edge_pose"], edge_point=o["edge_point"], edge_kind=o["edge_kind"], edge_obs=o["edge_obs"],
                      edge_info=o["edge_info"], lambda_init=0.0, max_iterations=max_iterations, kb8=self._last_kb8(),
                      cam2=self._last_rig()[0], trl=self._last_rig()[1]).normalise()
        # const float thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815) (src/Optimizer.cc:130-131); none unless bRobust
        w.huber_mono = float(np.float32(np.sqrt(5.99))) if robust else float("inf")
        w.huber_stereo = float(np.float32(np.sqrt(7.815))) if robust else float("inf")
        return w, o

    def run_gba(self, n_iterations=5, n_loop_kf=0, robust=True, stop_flag=None):
        rc = self.lib.osh_host_run_gba(self.g, n_iterations, capi.ptr(stop_flag, capi.c_uint8_p) if stop_flag is not None else
                                       C.cast(None, capi.c_uint8_p), int(n_loop_kf), int(robust))
        assert rc == 0

    # ---- welding Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag)
    def packed_welding_window(self, main, adjust, fixed):
        sizes = np.zeros(5, dtype=np.int32)
        d, i32, u8, i64 = capi.c_double_p, capi.c_int32_p, capi.c_uint8_p, capi.c_int64_p
        adj, fix = _i32(adjust), _i32(fixed)
        head = (self.g, int(main), len(adj), capi.ptr(adj, i32), len(fix), capi.ptr(fix, i32), capi.ptr(sizes, i32))
        rc = self.lib.osh_host_pack_welding(*head, *[C.cast(None, t) for t in (d, d, d, i32, i32, u8, d, d, i64, i64)])
        assert rc == 0, rc
        P, F, L, E = (int(x) for x in sizes[:4])
        o = dict(pose_qt=np.zeros((P + F, 7)), pose_cam=np.zeros((P + F, 5)), points=np.zeros((L, 3)),
                 edge_pose=np.zeros(E, dtype=np.int32), edge_point=np.zeros(E, dtype=np.int32), edge_kind=np.zeros(E, dtype=np.uint8),
                 edge_obs=np.zeros((E, 3)), edge_info=np.zeros(E), pose_kf_id=np.zeros(P + F, dtype=np.int64),
                 point_mp_id=np.zeros(L, dtype=np.int64))
        rc = self.lib.osh_host_pack_welding(*head, capi.ptr(o["pose_qt"], d), capi.ptr(o["pose_cam"], d), capi.ptr(o["points"], d),
                                            capi.ptr(o["edge_pose"], i32), capi.ptr(o["edge_point"], i32), capi.ptr(o["edge_kind"], u8),
                                            capi.ptr(o["edge_obs"], d), capi.ptr(o["edge_info"], d), capi.ptr(o["pose_kf_id"], i64),
                                            capi.ptr(o["point_mp_id"], i64))
        assert rc == 0, rc
        w = LbaWindow(n_free=P, n_fixed=F, pose_qt=o["pose_qt"], pose_cam=o["pose_cam"], points=o["points"],
                      edge_pose=o["edge_pose"], edge_point=o["edge_point"], edge_kind=o["edge_kind"], edge_obs=o["edge_obs"],
                      edge_info=o["edge_info"], lambda_init=0.0, max_iterations=5, kb8=self._last_kb8()).normalise()
        w.huber_mono = float(np.float32(np.sqrt(5.99)))      # const float thHuber2D = sqrt(5.99) (src/Optimizer.cc:3625)
        w.huber_stereo = float(np.float32(np.sqrt(7.815)))
        return w, o

    def run_welding(self, main, adjust, fixed, stop_flag=None):
        adj, fix = _i32(adjust), _i32(fixed)
        rc = self.lib.osh_host_run_welding(self.g, int(main), len(adj), capi.ptr(adj, capi.c_int32_p), len(fix), capi.ptr(fix, capi.c_int32_p),
                                           capi.ptr(stop_flag, capi.c_uint8_p) if stop_flag is not None else C.cast(None, capi.c_uint8_p))
        assert rc == 0

    def kf_pose_gba(self, i):
        o = np.zeros(7, dtype=np.float32)
        mark = self.lib.osh_host_get_kf_pose_gba(self.g, i, capi.ptr(o, capi.c_float_p))
        return int(mark), o

    def mp_pos_gba(self, j):
        o = np.zeros(3, dtype=np.float32)
        mark = self.lib.osh_host_get_mp_pos_gba(self.g, j, capi.ptr(o, capi.c_float_p))
        return int(mark), o

    def kf_pose(self, i):
        o = np.zeros(7, dtype=np.float32)
        self.lib.osh_host_get_kf_pose(self.g, i, capi.ptr(o, capi.c_float_p))
        return o

    def mp_pos(self, j):
        o = np.zeros(3, dtype=np.float32)
        self.lib.osh_host_get_mp_pos(self.g, j, capi.ptr(o, capi.c_float_p))
        return o

    # ---- the local-mapping steps: MapPoint::RefreshBatch, LocalMapping::SearchInNeighbors / ProcessNewKeyFrame
    def set_mapping(self, seed: int = 0, max_flips: int = 6, scale_factor: float = 1.2, n_levels: int = 8,
                    bounds=(0.0, 0.0, 752.0, 480.0), mb: float = 0.110078):
        """Descriptors (the parent descriptor of the observed point with up to max_flips bits flipped), level tables, image
        bounds and grid for every keyframe, and the first observing keyframe as every point's reference keyframe.  Keeps
        kf_desc[k] [rows, 32], kf_octave[k] and kf_point[k] [rows]: left keypoints in observation order, then the right ones of
        a rig."""
        w = self.w
        rng = np.random.default_rng(seed)
        body = w.edge_kind == capi.OSH_EDGE_BODY
        octave = np.round(np.log(1.0 / w.edge_info) / np.log(1.44)).astype(np.int32)
        n_kf = w.n_free + w.n_fixed
        parent = rng.integers(0, 256, (w.n_points, 32), dtype=np.uint8)
        self.kf_desc, self.kf_octave, self.kf_point = [], [], []
        for k in range(n_kf):
            rows = np.concatenate([np.flatnonzero(~body & (w.edge_pose == k)), np.flatnonzero(body & (w.edge_pose == k))])
            d = np.zeros((rows.size, 32), np.uint8)
            for i, e in enumerate(rows):
                bits = np.unpackbits(parent[w.edge_point[e]])
                bits[rng.choice(256, size=int(rng.integers(0, max_flips + 1)), replace=False)] ^= 1
                d[i] = np.packbits(bits)
            self.kf_desc.append(d)
            self.kf_octave.append(octave[rows].astype(np.int32))
            self.kf_point.append(np.asarray(w.edge_point)[rows].astype(np.int32))
        kf_rows = _i32([d.shape[0] for d in self.kf_desc])
        desc = np.ascontiguousarray(np.concatenate(self.kf_desc), np.uint8)
        self.scale_factors = np.ones(n_levels, np.float32)
        for level in range(1, n_levels):
            self.scale_factors[level] = self.scale_factors[level - 1] * np.float32(scale_factor)
        rc = self.lib.osh_host_graph_set_mapping(self.g, float(scale_factor), int(n_levels), capi.ptr(_f32(bounds), capi.c_float_p), float(mb),
                                                 capi.ptr(kf_rows, capi.c_int32_p), capi.ptr(desc, capi.c_uint8_p))
        assert rc == 0, rc
        first = np.full(w.n_points, n_kf, np.int32)
        np.minimum.at(first, np.asarray(w.edge_point), np.asarray(w.edge_pose, np.int32))
        first[first == n_kf] = -1
        self.set_ref_kf(np.arange(w.n_points), first)

    def set_ref_kf(self, mp, kf):
        mp, kf = _i32(mp), _i32(kf)
        assert self.lib.osh_host_graph_set_ref_kf(self.g, mp.shape[0], capi.ptr(mp, capi.c_int32_p), capi.ptr(kf, capi.c_int32_p)) == 0

    def unlink(self, kf: int, mp: int, keep_match: bool = False):
        assert self.lib.osh_host_graph_unlink(self.g, int(kf), int(mp), int(keep_match)) == 0

    def clone_point(self, mp: int, new_id: int, kfs) -> int:
        kfs = _i32(kfs)
        j = self.lib.osh_host_graph_clone_point(self.g, int(mp), int(new_id), kfs.shape[0], capi.ptr(kfs, capi.c_int32_p))
        assert j >= 0
        return j

    def refresh_batch(self, mps):
        """MapPoint::RefreshBatch on the points listed (-1: a null entry)."""
        mps = _i32(mps)
        assert self.lib.osh_host_mp_refresh_batch(self.g, mps.shape[0], capi.ptr(mps, capi.c_int32_p)) == 0

    def refresh_pack(self, mps) -> dict:
        """What RefreshBatch packs for the list, without a device."""
        mps = _i32(mps)
        sizes = np.zeros(3, np.int32)
        pointer = {np.dtype(np.int32): capi.c_int32_p, np.dtype(np.uint8): capi.c_uint8_p, np.dtype(np.float32): capi.c_float_p}
        call = lambda arrays: self.lib.osh_host_mp_refresh_pack(self.g, mps.shape[0], capi.ptr(mps, capi.c_int32_p), capi.ptr(sizes, capi.c_int32_p), *arrays)
        types = (np.int32,) * 4 + (np.uint8, np.int32, np.uint8, np.float32, np.float32, np.int32, np.float32, np.float32)
        assert call([C.cast(None, pointer[np.dtype(t)]) for t in types]) == 0
        P, E, Cn = (int(x) for x in sizes)
        o = dict(point_mp=np.zeros(P, np.int32), entry_off=np.zeros(P + 1, np.int32), entry_kf=np.zeros(E, np.int32),
                 entry_row=np.zeros(E, np.int32), desc=np.zeros((E, 32), np.uint8), centre=np.zeros(E, np.int32),
                 use_desc=np.zeros(E, np.uint8), centres=np.zeros((Cn, 3), np.float32), pos=np.zeros((P, 3), np.float32),
                 ref_centre=np.zeros(P, np.int32), level_scale=np.zeros(P, np.float32), top_scale=np.zeros(P, np.float32))
        assert call([capi.ptr(v, pointer[v.dtype]) for v in o.values()]) == 0
        return o

    def mp_refresh(self, j: int) -> dict:
        """mDescriptor, mNormalVector, the two distances and the two update counters of point j."""
        desc, normal, mm, counts = np.zeros(32, np.uint8), np.zeros(3, np.float32), np.zeros(2, np.float32), np.zeros(2, np.int32)
        has = self.lib.osh_host_mp_get_refresh(self.g, int(j), capi.ptr(desc, capi.c_uint8_p), capi.ptr(normal, capi.c_float_p),
                                               capi.ptr(mm, capi.c_float_p), capi.ptr(counts, capi.c_int32_p))
        assert has >= 0
        return dict(has_desc=bool(has), desc=desc, normal=normal, min_distance=mm[0], max_distance=mm[1],
                    desc_updates=int(counts[0]), normal_updates=int(counts[1]))

    def mp_observations(self, j: int) -> list:
        """(keyframe index, left index, right index) in the order the reference walks mObservations."""
        n = self.lib.osh_host_mp_observations(self.g, int(j), 0, *[C.cast(None, capi.c_int32_p)] * 3)
        kf, left, right = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        self.lib.osh_host_mp_observations(self.g, int(j), n, *[capi.ptr(a, capi.c_int32_p) for a in (kf, left, right)])
        return [(int(kf[i]), int(left[i]), int(right[i])) for i in range(n)]

    def mp_state(self, j: int) -> dict:
        o = np.zeros(4, np.int64)
        assert self.lib.osh_host_mp_state(self.g, int(j), capi.ptr(o, capi.c_int64_p)) == 0
        return dict(bad=bool(o[0]), replaced=int(o[1]), fuse_candidate_for=int(o[2]), ref_kf=int(o[3]))

    def kf_matches(self, k: int) -> np.ndarray:
        n = self.lib.osh_host_kf_matches(self.g, int(k), 0, C.cast(None, capi.c_int32_p))
        mp = np.zeros(max(n, 1), np.int32)
        self.lib.osh_host_kf_matches(self.g, int(k), n, capi.ptr(mp, capi.c_int32_p))
        return mp[:n]

    def kf_state(self, k: int) -> dict:
        marks, centres = np.zeros(3, np.int64), np.zeros(6, np.float32)
        assert self.lib.osh_host_kf_state(self.g, int(k), capi.ptr(marks, capi.c_int64_p), capi.ptr(centres, capi.c_float_p)) == 0
        return dict(fuse_target_for=int(marks[0]), connection_updates=int(marks[1]), n_left=int(marks[2]), centres=centres.reshape(2, 3))

    def fuse(self, kf: int, mps, th: float = 3.0, right: bool = False) -> int:
        mps = _i32(mps)
        return self.lib.osh_host_graph_fuse(self.g, int(kf), mps.shape[0], capi.ptr(mps, capi.c_int32_p), float(th), int(right))

    def fuse_batch(self, targets, mps, cpu_search: bool = False):
        """ORBmatcher::FuseBatch(targets, vpMapPoints): targets = [(keyframe, th, right)].  Returns the counts and (mnFuseBatchResearched, mnFuseBatchResearchedChanged)."""
        mps, kf = _i32(mps), _i32([t[0] for t in targets])
        th, right = _f32([t[1] for t in targets]), np.ascontiguousarray([t[2] for t in targets], dtype=np.uint8)
        fused, researched = np.zeros(max(len(targets), 1), np.int32), np.zeros(2, np.int32)
        rc = self.lib.osh_host_graph_fuse_batch(self.g, len(targets), capi.ptr(kf, capi.c_int32_p), capi.ptr(th, capi.c_float_p), capi.ptr(right, capi.c_uint8_p),
                                                mps.shape[0], capi.ptr(mps, capi.c_int32_p), int(cpu_search), capi.ptr(fused, capi.c_int32_p), capi.ptr(researched, capi.c_int32_p))
        assert rc == 0
        return fused[:len(targets)].tolist(), (int(researched[0]), int(researched[1]))

    def fuse_batch_sim3(self, targets, mps, th: float = 4.0, cpu_search: bool = False, replace_after: bool = False):
        """The Sim3 overload: targets = [(keyframe, sim3 of 8 floats qw qx qy qz tx ty tz s)].  Returns the counts, the vpReplacePoint
        lists [targets, points] as point indices and mnFuseBatchResearched."""
        mps, kf = _i32(mps), _i32([t[0] for t in targets])
        sim3 = _f32(np.array([t[1] for t in targets]).reshape(-1))
        n_t, n = len(targets), mps.shape[0]
        fused, replace, researched = np.zeros(max(n_t, 1), np.int32), np.full(max(n_t * n, 1), -1, np.int32), np.zeros(2, np.int32)
        rc = self.lib.osh_host_graph_fuse_batch_sim3(self.g, n_t, capi.ptr(kf, capi.c_int32_p), capi.ptr(sim3, capi.c_float_p), n, capi.ptr(mps, capi.c_int32_p),
                                                     float(th), int(cpu_search), int(replace_after), capi.ptr(fused, capi.c_int32_p),
                                                     capi.ptr(replace, capi.c_int32_p), capi.ptr(researched, capi.c_int32_p))
        assert rc == 0
        return fused[:n_t].tolist(), replace[:n_t * n].reshape(n_t, n), (int(researched[0]), int(researched[1]))

    def fuse_sim3(self, kf: int, sim3, mps, th: float = 4.0):
        """One ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): the count and the list as point indices."""
        mps, s = _i32(mps), _f32(np.asarray(sim3))
        replace = np.full(max(mps.shape[0], 1), -1, np.int32)
        n = self.lib.osh_host_graph_fuse_sim3(self.g, int(kf), capi.ptr(s, capi.c_float_p), mps.shape[0], capi.ptr(mps, capi.c_int32_p), float(th),
                                              capi.ptr(replace, capi.c_int32_p))
        assert n >= 0
        return n, replace[:mps.shape[0]]

    def fuse_candidates(self, kf: int, mps, th: float = 3.0, right: bool = False, sim3=None):
        """What one ORBmatcher::Fuse call decides per point before its device search: count [n] (-1: no query) and the candidate
        lists, one per query in point order, as indices in the keyframe's own arrays."""
        mps = _i32(mps)
        s = None if sim3 is None else _f32(np.asarray(sim3))
        count = np.zeros(max(mps.shape[0], 1), np.int32)
        args = (self.g, int(kf), capi.ptr(s, capi.c_float_p), float(th), int(right), mps.shape[0], capi.ptr(mps, capi.c_int32_p), capi.ptr(count, capi.c_int32_p))
        total = self.lib.osh_host_graph_fuse_candidates(*args, 0, C.cast(None, capi.c_int32_p))
        assert total >= 0
        cand = np.zeros(max(total, 1), np.int32)
        assert self.lib.osh_host_graph_fuse_candidates(*args, total, capi.ptr(cand, capi.c_int32_p)) == total
        count = count[:mps.shape[0]]
        lists, at = [], 0
        for c in count:
            lists.append(None if c < 0 else cand[at:at + c].copy())
            at += max(int(c), 0)
        return count, lists

    def fuse_pack_search(self, kf: int, mps, th: float = 3.0, right: bool = False, sim3=None, cpu_search: bool = False) -> dict:
        """The same call as FuseBatch packs and searches it: stage, n_candidates, best_idx (keyframe's own arrays), best_dist [n]."""
        mps = _i32(mps)
        s = None if sim3 is None else _f32(np.asarray(sim3))
        out = {k: np.zeros(max(mps.shape[0], 1), np.int32) for k in ("stage", "n_candidates", "best_idx", "best_dist")}
        rc = self.lib.osh_host_graph_fuse_pack_search(self.g, int(kf), capi.ptr(s, capi.c_float_p), float(th), int(right), mps.shape[0],
                                                      capi.ptr(mps, capi.c_int32_p), int(cpu_search), *[capi.ptr(v, capi.c_int32_p) for v in out.values()])
        assert rc == 0, rc
        return {k: v[:mps.shape[0]] for k, v in out.items()}

    def replace(self, mp: int, by: int):
        assert self.lib.osh_host_graph_replace(self.g, int(mp), int(by)) == 0

    def loop_search_and_fuse(self, kfs, mps, sim3=None, cpu_search: bool = False):
        """LoopClosing::SearchAndFuse: with sim3 [len(kfs), 8] the KeyFrameAndPose overload, else the keyframe-list one.  Returns the
        order the keyframes were walked in, the replacements made and mnFuseBatchResearched."""
        kfs, mps = _i32(kfs), _i32(mps)
        s = None if sim3 is None else np.ascontiguousarray(np.asarray(sim3, np.float64).reshape(-1))
        order, info = np.zeros(max(kfs.shape[0], 1), np.int32), np.zeros(3, np.int32)
        rc = self.lib.osh_host_loop_search_and_fuse(self.g, int(s is not None), kfs.shape[0], capi.ptr(kfs, capi.c_int32_p), capi.ptr(s, capi.c_double_p),
                                                    mps.shape[0], capi.ptr(mps, capi.c_int32_p), int(cpu_search), capi.ptr(order, capi.c_int32_p),
                                                    capi.ptr(info, capi.c_int32_p))
        assert rc == 0
        return order[:kfs.shape[0]].tolist(), int(info[0]), (int(info[1]), int(info[2]))

    def set_covisible(self, kf: int, others):
        others = _i32(others)
        assert self.lib.osh_host_graph_set_covisible(self.g, int(kf), others.shape[0], capi.ptr(others, capi.c_int32_p)) == 0

    def set_bad(self, kf: int = -1, mp: int = -1):
        self.lib.osh_host_set_bad(self.g, int(kf), int(mp))

    def search_in_neighbors(self, kf: int | None = None, monocular: bool = False, inertial: bool = False, abort_ba: bool = False):
        kf = self.cur if kf is None else kf
        assert self.lib.osh_host_local_mapping_search_in_neighbors(self.g, int(kf), int(monocular), int(inertial), int(abort_ba)) == 0

    def process_new_keyframe(self, kf: int) -> dict:
        recent, in_map = np.zeros(4096, np.int32), C.c_int32(0)
        n = self.lib.osh_host_local_mapping_process_new_keyframe(self.g, int(kf), recent.shape[0], capi.ptr(recent, capi.c_int32_p), C.byref(in_map))
        assert n >= 0
        return dict(recent=recent[:n].copy(), in_map=int(in_map.value))


class HostCullGraph:
    """The stand-in map of a synth_keyframe_cull.CullScene (osh_host_cull_graph_create) for LocalMapping::KeyFrameCulling,
    MapPointCulling and PackKeyFrameCull.  Keyframe and point indices are those of the scene."""

    def __init__(self, sc):
        self.lib = capi.load_host_library()
        self.sc = sc
        kfs = sc.kfs
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
        slots = [s for kf in kfs for s in kf["slots"]]
        a = dict(
            kf_id=np.ascontiguousarray([kf["id"] for kf in kfs], dtype=np.int64), kf_n_slots=_i32([len(kf["slots"]) for kf in kfs]),
            kf_n_left=_i32([kf["n_left"] for kf in kfs]), kf_camera2=u8([kf["camera2"] for kf in kfs]),
            kf_th_depth=_f32([kf["th_depth"] for kf in kfs]), kf_timestamp=np.ascontiguousarray([kf["timestamp"] for kf in kfs], dtype=np.float64),
            kf_not_erase=u8([kf["not_erase"] for kf in kfs]), kf_bad=u8([kf["bad"] for kf in kfs]),
            kf_imu_pos=_f32([kf["imu_pos"] for kf in kfs]).reshape(-1), kf_prev=_i32([kf["prev"] for kf in kfs]), kf_next=_i32([kf["next"] for kf in kfs]),
            kf_has_preint=u8([kf["preint"] for kf in kfs]), slot_point=_i32([s[0] for s in slots]).reshape(-1), slot_octave=_i32([s[1] for s in slots]).reshape(-1),
            slot_u_right=_f32([s[2] for s in slots]).reshape(-1), slot_depth=_f32([s[3] for s in slots]).reshape(-1),
            mp_n_obs=_i32([sc.mp_n_obs.get(j, -1) for j in range(sc.n_mp)]).reshape(-1), mp_bad=u8([j in sc.mp_bad for j in range(sc.n_mp)]))
        c = capi.HostCullScene()
        c.n_kf, c.n_mp = len(kfs), sc.n_mp
        c.init_kf_id, c.keyframes_in_map = int(sc.init_kf_id), int(sc.keyframes_in_map)
        c.imu_initialized, c.inertial_ba2 = int(sc.imu_initialized), int(sc.inertial_ba2)
        types = dict(capi.HostCullScene._fields_)
        for name, arr in a.items():
            setattr(c, name, capi.ptr(arr, types[name]))
        self.g = C.c_void_p(self.lib.osh_host_cull_graph_create(C.byref(c)))
        if not self.g:
            raise RuntimeError("osh_host_cull_graph_create refused the scene")
        if sc.current is not None:
            cov = _i32(sc.covisible).reshape(-1)
            self.lib.osh_host_graph_set_covisible(self.g, sc.current, len(cov), capi.ptr(cov, capi.c_int32_p))

    def close(self):
        if self.g:
            self.lib.osh_host_graph_destroy(self.g)
            self.g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def keyframe_culling(self) -> dict:
        """LocalMapping::KeyFrameCulling with the scene's current keyframe and flags: the culled keyframes in list order and the
        number of osh_orb_keyframe_cull_count calls.  The wrapper's check of the state rule against the objects raises here."""
        sc = self.sc
        culled = np.full(max(1, len(sc.covisible)), -1, dtype=np.int32)
        calls = C.c_int32(-1)
        n = self.lib.osh_host_local_mapping_keyframe_culling(self.g, sc.current, int(sc.monocular), int(sc.inertial), int(sc.abort_ba), len(culled),
                                                             capi.ptr(culled, capi.c_int32_p), C.byref(calls))
        if n == -2:
            raise AssertionError("the state rule of keyframe_cull.h disagrees with the map points after SetBadFlag")
        if n < 0:
            raise RuntimeError(f"osh_host_local_mapping_keyframe_culling -> {n}")
        return {"culled": [int(k) for k in culled[:n]], "device_calls": int(calls.value)}

    def pack(self, candidates=None, monocular=None, objects: bool = True) -> dict:
        """PackKeyFrameCull for a candidate list (default: the scene's covisibility list), as tests/keyframe_cull_numpy.pack.
        objects=False leaves out table_kf and point_mp (a linear search per entry)."""
        cand = _i32(self.sc.covisible if candidates is None else candidates).reshape(-1)
        mono = int(self.sc.monocular if monocular is None else monocular)
        sizes = np.zeros(4, dtype=np.int32)
        nul = [None] * 12

        def call(arrs):
            rc = self.lib.osh_host_kfcull_pack(self.g, len(cand), capi.ptr(cand, capi.c_int32_p), mono, capi.ptr(sizes, capi.c_int32_p),
                                               *[capi.ptr(x, capi.c_uint8_p if i == 7 else capi.c_int32_p) for i, x in enumerate(arrs)])
            assert rc == 0, rc
        call(nul)
        T, S, P, E = (int(x) for x in sizes)
        names = ["table_kf", "cand_slot_off", "slot_point", "slot_level", "slot_index", "point_mp", "point_n_obs", "point_bad", "point_obs_off",
                 "obs_kf", "obs_level", "obs_weight"]
        shape = [T, len(cand) + 1, S, S, S, P, P, P, P + 1, E, E, E]
        arrs = [np.zeros(n, dtype=np.uint8 if name == "point_bad" else np.int32) for name, n in zip(names, shape)]
        call([None if (not objects and name in ("table_kf", "point_mp")) else x for name, x in zip(names, arrs)])
        return dict(zip(names, arrs))

    def pack_and_reference_times(self, candidates=None, monocular=None) -> dict:
        """osh_host_kfcull_time: the wall time of PackKeyFrameCull and of the reference-shaped counting loop, with that loop's totals."""
        cand = _i32(self.sc.covisible if candidates is None else candidates).reshape(-1)
        mono = int(self.sc.monocular if monocular is None else monocular)
        ms, totals = np.zeros(2, dtype=np.float64), np.zeros(2, dtype=np.int64)
        rc = self.lib.osh_host_kfcull_time(self.g, len(cand), capi.ptr(cand, capi.c_int32_p), mono, capi.ptr(ms, capi.c_double_p), capi.ptr(totals, capi.c_int64_p))
        assert rc == 0, rc
        return {"pack_ms": float(ms[0]), "reference_loop_ms": float(ms[1]), "n_mps": int(totals[0]), "n_redundant": int(totals[1])}

    def kf_state(self, k: int) -> dict:
        out = np.zeros(9, dtype=np.int64)
        assert self.lib.osh_host_kf_cull_state(self.g, int(k), capi.ptr(out, capi.c_int64_p)) == 0
        names = ["bad", "to_be_erased", "prev", "next", "best_covisible_updates", "connection_erasures", "spanning_tree_updates", "merged_previous", "merges"]
        return dict(zip(names, (int(x) for x in out)))

    def mp_state(self, j: int) -> dict:
        out = np.zeros(3, dtype=np.int64)
        assert self.lib.osh_host_mp_cull_state(self.g, int(j), capi.ptr(out, capi.c_int64_p)) == 0
        return {"n_obs": int(out[0]), "bad": int(out[1]), "observers": int(out[2])}

    def set_point_culling(self, j: int, first_kf_id: int, n_visible: int, n_found: int):
        assert self.lib.osh_host_mp_set_culling(self.g, int(j), int(first_kf_id), int(n_visible), int(n_found)) == 0

    def map_point_culling(self, kf: int, points, monocular: bool) -> list:
        """LocalMapping::MapPointCulling with mlpRecentAddedMapPoints = points: the list afterwards."""
        pts = _i32(points).reshape(-1)
        rem = np.full(max(1, len(pts)), -1, dtype=np.int32)
        n = self.lib.osh_host_local_mapping_map_point_culling(self.g, int(kf), int(monocular), len(pts), capi.ptr(pts, capi.c_int32_p), len(rem),
                                                              capi.ptr(rem, capi.c_int32_p))
        assert n >= 0, n
        return [int(x) for x in rem[:n]]


class HostFrame:
    def __init__(self, xy, octave, desc, angle=None, uright=None, pose_qt=None, mbf=float(synth.BF), mb=0.110078, kb8=None):
        self.lib = capi.load_host_library()
        n = len(octave)
        self.n = n
        pose = _f32(pose_qt if pose_qt is not None else [0, 0, 0, 1, 0, 0, 0])
        cam4 = _f32([synth.FX, synth.FY, synth.CX, synth.CY])
        a = _f32(angle) if angle is not None else None
        u = _f32(uright) if uright is not None else None
        self.f = C.c_void_p(self.lib.osh_host_frame_create(
            n, capi.ptr(_f32(xy), capi.c_float_p), capi.ptr(_i32(octave), capi.c_int32_p),
            capi.ptr(a, capi.c_float_p) if a is not None else C.cast(None, capi.c_float_p),
            capi.ptr(u, capi.c_float_p) if u is not None else C.cast(None, capi.c_float_p),
            capi.ptr(np.ascontiguousarray(desc, dtype=np.uint8), capi.c_uint8_p), capi.ptr(pose, capi.c_float_p),
            capi.ptr(cam4, capi.c_float_p), mbf, mb, synth.N_LEVELS, np.float32(synth.SCALE_FACTOR)))
        if kb8 is not None:      # monocular fisheye frame: mpCamera is a KannalaBrandt8
            self.lib.osh_host_frame_set_fisheye(self.f, capi.ptr(_f32(kb8), capi.c_float_p))

    def close(self):
        if self.f:
            self.lib.osh_host_frame_destroy(self.f)
            self.f = C.c_void_p()

    def set_rig(self, n_left, left_to_right, right_to_left, trl=(0, 0, 0, 1, -0.1, 0, 0)):
        """Fisheye stereo layout: keypoints [0, n_left) left camera, the rest right camera."""
        keep = [_i32(left_to_right), _i32(right_to_left), _f32(np.asarray(trl))]
        rc = self.lib.osh_host_frame_set_rig(self.f, int(n_left), capi.ptr(keep[0], capi.c_int32_p), capi.ptr(keep[1], capi.c_int32_p),
                                             capi.ptr(keep[2], capi.c_float_p))
        assert rc == 0

    def search_local_points_rig(self, mp_desc, in_l, proj_l, level_l, viewcos_l, in_r, proj_r, level_r, viewcos_r, n_obs=None, nnratio=0.8, th=1.0):
        n_mp = len(mp_desc)
        assign = -np.ones(self.n, dtype=np.int32)
        keep = [np.ascontiguousarray(mp_desc, dtype=np.uint8), np.ascontiguousarray(in_l, dtype=np.uint8), _f32(proj_l), _i32(level_l), _f32(viewcos_l),
                np.ascontiguousarray(in_r, dtype=np.uint8), _f32(proj_r), _i32(level_r), _f32(viewcos_r),
                _i32(n_obs) if n_obs is not None else None]
        u8, fp, i32 = capi.c_uint8_p, capi.c_float_p, capi.c_int32_p
        n = self.lib.osh_host_search_local_points_rig(self.f, n_mp, capi.ptr(keep[0], u8), capi.ptr(keep[1], u8), capi.ptr(keep[2], fp),
                                                      capi.ptr(keep[3], i32), capi.ptr(keep[4], fp), capi.ptr(keep[5], u8), capi.ptr(keep[6], fp),
                                                      capi.ptr(keep[7], i32), capi.ptr(keep[8], fp), capi.ptr(keep[9], i32), nnratio, th,
                                                      capi.ptr(assign, i32))
        return int(n), assign

    def search_local_points(self, mp_desc, proj_xy, level, viewcos=None, proj_xr=None, depth=None, n_obs=None, nnratio=0.8, th=1.0):
        n_mp = len(level)
        assign = -np.ones(self.n, dtype=np.int32)
        fp = capi.c_float_p

        def opt(a, typ, conv):
            return capi.ptr(conv(a), typ) if a is not None else C.cast(None, typ)
        keep = [np.ascontiguousarray(mp_desc, dtype=np.uint8), _f32(proj_xy), _i32(level)]
        n = self.lib.osh_host_search_local_points(self.f, n_mp, capi.ptr(keep[0], capi.c_uint8_p), capi.ptr(keep[1], fp),
                                                  opt(proj_xr, fp, _f32), capi.ptr(keep[2], capi.c_int32_p), opt(viewcos, fp, _f32),
                                                  opt(depth, fp, _f32), opt(n_obs, capi.c_int32_p, _i32), nnratio, th,
                                                  capi.ptr(assign, capi.c_int32_p))
        return n, assign

    def search_local_points_projected(self, mp_pos, mp_normal, mp_min_dist, mp_max_dist, viewing_cos_limit=0.5, mp_desc=None,
                                      n_obs=None, nnratio=0.8, th=1.0):
        """Frame::isInFrustum for every map point on the device (src/Frame.cc:513-587), then, when descriptors are given,
        SearchByProjection(F, vpMapPoints, th) as in Tracking::SearchLocalPoints (src/Tracking.cc:3411-3460)."""
        n_mp = len(mp_min_dist)
        fp, ip = capi.c_float_p, capi.c_int32_p
        keep = [_f32(mp_pos), _f32(mp_normal), _f32(mp_min_dist), _f32(mp_max_dist)]
        out = dict(in_view=np.zeros(n_mp, np.uint8), proj_xy=np.zeros((n_mp, 2), np.float32), proj_xr=np.zeros(n_mp, np.float32),
                   depth=np.zeros(n_mp, np.float32), view_cos=np.zeros(n_mp, np.float32), level=np.zeros(n_mp, np.int32))
        assign = -np.ones(self.n, dtype=np.int32) if mp_desc is not None else None
        nm = C.c_int32(0)
        desc = np.ascontiguousarray(mp_desc, dtype=np.uint8) if mp_desc is not None else None
        nobs = _i32(n_obs) if n_obs is not None else None
        n_in = self.lib.osh_host_frame_search_local_points_projected(
            self.f, n_mp, capi.ptr(keep[0], fp), capi.ptr(keep[1], fp), capi.ptr(keep[2], fp), capi.ptr(keep[3], fp), viewing_cos_limit,
            capi.ptr(out["in_view"], capi.c_uint8_p), capi.ptr(out["proj_xy"], fp), capi.ptr(out["proj_xr"], fp), capi.ptr(out["depth"], fp),
            capi.ptr(out["view_cos"], fp), capi.ptr(out["level"], ip), capi.ptr(desc, capi.c_uint8_p), capi.ptr(nobs, ip), nnratio, th,
            capi.ptr(assign, ip), C.cast(C.byref(nm), ip) if assign is not None else C.cast(None, ip))
        if n_in < 0:
            raise RuntimeError("osh_host_frame_search_local_points_projected failed: " + capi.last_error())
        out.update(n_in_view=n_in, assignment=assign, n_matches=nm.value)
        return out

    def search_last_frame(self, last: "HostFrame", last_mp, mp_pos, mp_desc, th=15.0, mono=True, check_ori=True):
        assign = -np.ones(self.n, dtype=np.int32)
        keep = [_i32(last_mp), _f32(mp_pos), np.ascontiguousarray(mp_desc, dtype=np.uint8)]
        n = self.lib.osh_host_search_last_frame(self.f, last.f, capi.ptr(keep[0], capi.c_int32_p), len(mp_pos),
                                                capi.ptr(keep[1], capi.c_float_p), capi.ptr(keep[2], capi.c_uint8_p), th, int(mono),
                                                int(check_ori), capi.ptr(assign, capi.c_int32_p))
        return n, assign


    def search_keyframe(self, kf_angle, kf_mp, mp_pos, mp_desc, mp_min_max_dist, mp_found=None, mp_bad=None, cur_mp=None,
                        th=10.0, orb_dist=100, check_ori=True):
        """ORBmatcher(0.9, check_ori).SearchByProjection(self, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1889-2010)."""
        assign = -np.ones(self.n, dtype=np.int32)
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        keep = [_f32(kf_angle), _i32(kf_mp), _f32(mp_pos), u8(mp_desc), _f32(mp_min_max_dist),
                u8(mp_found if mp_found is not None else np.zeros(len(mp_pos))), u8(mp_bad if mp_bad is not None else np.zeros(len(mp_pos))),
                _i32(cur_mp if cur_mp is not None else -np.ones(self.n))]
        n = self.lib.osh_host_search_keyframe(self.f, len(kf_mp), capi.ptr(keep[0], capi.c_float_p), capi.ptr(keep[1], capi.c_int32_p),
                                              len(mp_pos), capi.ptr(keep[2], capi.c_float_p), capi.ptr(keep[3], capi.c_uint8_p),
                                              capi.ptr(keep[4], capi.c_float_p), capi.ptr(keep[5], capi.c_uint8_p),
                                              capi.ptr(keep[6], capi.c_uint8_p), capi.ptr(keep[7], capi.c_int32_p), th, int(orb_dist),
                                              int(check_ori), capi.ptr(assign, capi.c_int32_p))
        return n, assign


    def search_by_bow(self, kf_desc, kf_angle, kf_has_mp, kf_fv, f_fv, nnratio=0.7, check_ori=True):
        """ORBmatcher(nnratio, check_ori).SearchByBoW(pKF, F, vpMapPointMatches) (src/ORBmatcher.cc:223-420).  kf_fv / f_fv: feature
        vectors as (node_id[n], node_off[n + 1], node_feat) with ascending node ids.  Returns (nmatches, assignment[F.N])."""
        kf_desc = np.ascontiguousarray(kf_desc, dtype=np.uint8)
        keep = [kf_desc, _f32(kf_angle), np.ascontiguousarray(kf_has_mp, dtype=np.uint8)] + [_i32(a) for a in kf_fv] + [_i32(a) for a in f_fv]
        assign = np.zeros(self.n, dtype=np.int32)
        n = self.lib.osh_host_search_by_bow(self.f, len(kf_desc), capi.ptr(keep[0], capi.c_uint8_p), capi.ptr(keep[1], capi.c_float_p),
                                            capi.ptr(keep[2], capi.c_uint8_p), len(keep[3]), capi.ptr(keep[3], capi.c_int32_p),
                                            capi.ptr(keep[4], capi.c_int32_p), capi.ptr(keep[5], capi.c_int32_p), len(keep[6]),
                                            capi.ptr(keep[6], capi.c_int32_p), capi.ptr(keep[7], capi.c_int32_p), capi.ptr(keep[8], capi.c_int32_p),
                                            float(nnratio), int(check_ori), capi.ptr(assign, capi.c_int32_p))
        return n, assign

    def set_camera2(self, cam2):
        """Give the right camera of a fisheye stereo frame its own KannalaBrandt8 (fx fy cx cy k1..k4)."""
        assert self.lib.osh_host_frame_set_camera2(self.f, capi.ptr(_f32(cam2), capi.c_float_p)) == 0

    def pose_optimization(self, kp_mp, mp_pos):
        """Optimizer::PoseOptimization(&frame) (src/Optimizer.cc:815-1114); returns (n_inliers, pose_qt, mvbOutlier)."""
        pose = np.zeros(7, dtype=np.float32)
        outlier = np.zeros(self.n, dtype=np.uint8)
        keep = [_f32(mp_pos), _i32(kp_mp), _f32(synth.INV_LEVEL_SIGMA2)]
        n = self.lib.osh_host_frame_pose_optimization(self.f, len(mp_pos), capi.ptr(keep[0], capi.c_float_p), capi.ptr(keep[1], capi.c_int32_p),
                                                      capi.ptr(keep[2], capi.c_float_p), len(keep[2]), capi.ptr(pose, capi.c_float_p),
                                                      capi.ptr(outlier, capi.c_uint8_p))
        return n, pose, outlier

    def search_sim3(self, scw, mp_pos, mp_desc, mp_min_max_dist, mp_normal, mp_bad=None, matched_in=None, th=3, ratio_hamming=1.0,
                    with_keyframes=False):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming)
        (src/ORBmatcher.cc:427-646) with this frame turned into the keyframe."""
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        out, out_kf = -np.ones(self.n, dtype=np.int32), -np.ones(self.n, dtype=np.int32)
        keep = [_f32(scw), _f32(mp_pos), u8(mp_desc), _f32(mp_min_max_dist), _f32(mp_normal),
                u8(mp_bad if mp_bad is not None else np.zeros(len(mp_pos))), _i32(matched_in if matched_in is not None else -np.ones(self.n))]
        fp = capi.c_float_p
        n = self.lib.osh_host_search_sim3(self.f, capi.ptr(keep[0], fp), len(mp_pos), capi.ptr(keep[1], fp), capi.ptr(keep[2], capi.c_uint8_p),
                                          capi.ptr(keep[3], fp), capi.ptr(keep[4], fp), capi.ptr(keep[5], capi.c_uint8_p),
                                          capi.ptr(keep[6], capi.c_int32_p), int(th), float(ratio_hamming), int(with_keyframes),
                                          capi.ptr(out, capi.c_int32_p), capi.ptr(out_kf, capi.c_int32_p))
        return n, out, out_kf


    def fuse(self, mp_pos, mp_desc, mp_min_max_dist, mp_normal, mp_nobs, slot_res, res_nobs, mp_bad=None, null_mask=None, res_bad=None, th=3.0):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:1148-1338) with this frame turned into the keyframe.  Returns
        nFused and a dict: slot (the keyframe's matches afterwards), cand_bad / cand_replaced / cand_nobs, res_bad / res_replaced /
        res_nobs (ids: candidate j -> j, resident r -> 100000 + r, none -> -1)."""
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        n_mp, n_res = len(mp_pos), len(res_nobs)
        zeros = np.zeros(max(n_mp, n_res, 1))
        keep = [_f32(mp_pos), u8(mp_desc), _f32(mp_min_max_dist), _f32(mp_normal), u8(mp_bad if mp_bad is not None else zeros[:n_mp]),
                u8(null_mask if null_mask is not None else zeros[:n_mp]), _i32(mp_nobs), _i32(slot_res), _i32(res_nobs),
                u8(res_bad if res_bad is not None else zeros[:n_res])]
        out = dict(slot=-np.ones(self.n, dtype=np.int32), cand_bad=np.zeros(n_mp, dtype=np.uint8), cand_replaced=-np.ones(n_mp, dtype=np.int32),
                   cand_nobs=np.zeros(n_mp, dtype=np.int32), res_bad=np.zeros(max(n_res, 1), dtype=np.uint8),
                   res_replaced=-np.ones(max(n_res, 1), dtype=np.int32), res_nobs=np.zeros(max(n_res, 1), dtype=np.int32))
        fp, ip, bp = capi.c_float_p, capi.c_int32_p, capi.c_uint8_p
        n = self.lib.osh_host_fuse(self.f, n_mp, capi.ptr(keep[0], fp), capi.ptr(keep[1], bp), capi.ptr(keep[2], fp), capi.ptr(keep[3], fp),
                                   capi.ptr(keep[4], bp), capi.ptr(keep[5], bp), capi.ptr(keep[6], ip), n_res, capi.ptr(keep[7], ip),
                                   capi.ptr(keep[8], ip), capi.ptr(keep[9], bp), float(th), capi.ptr(out["slot"], ip), capi.ptr(out["cand_bad"], bp),
                                   capi.ptr(out["cand_replaced"], ip), capi.ptr(out["cand_nobs"], ip), capi.ptr(out["res_bad"], bp),
                                   capi.ptr(out["res_replaced"], ip), capi.ptr(out["res_nobs"], ip))
        for k in ("res_bad", "res_replaced", "res_nobs"):
            out[k] = out[k][:n_res]
        return n, out


    def fuse_sim3(self, scw, mp_pos, mp_desc, mp_min_max_dist, mp_normal, mp_nobs, slot_res, n_res, mp_bad=None, found_slot=None, res_bad=None, th=3.0):
        """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1340-1455) with this frame turned into the
        keyframe.  Returns nFused, the keyframe's matches afterwards, vpReplacePoint as ids, Observations() of the candidates."""
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        n_mp = len(mp_pos)
        keep = [_f32(scw), _f32(mp_pos), u8(mp_desc), _f32(mp_min_max_dist), _f32(mp_normal), u8(mp_bad if mp_bad is not None else np.zeros(n_mp)),
                _i32(mp_nobs), _i32(found_slot if found_slot is not None else -np.ones(n_mp)), _i32(slot_res),
                u8(res_bad if res_bad is not None else np.zeros(max(n_res, 1)))]
        slot, repl, nobs = -np.ones(self.n, dtype=np.int32), -np.ones(n_mp, dtype=np.int32), np.zeros(n_mp, dtype=np.int32)
        fp, ip, bp = capi.c_float_p, capi.c_int32_p, capi.c_uint8_p
        n = self.lib.osh_host_fuse_sim3(self.f, capi.ptr(keep[0], fp), n_mp, capi.ptr(keep[1], fp), capi.ptr(keep[2], bp), capi.ptr(keep[3], fp),
                                        capi.ptr(keep[4], fp), capi.ptr(keep[5], bp), capi.ptr(keep[6], ip), capi.ptr(keep[7], ip), int(n_res),
                                        capi.ptr(keep[8], ip), capi.ptr(keep[9], bp), float(th), capi.ptr(slot, ip), capi.ptr(repl, ip), capi.ptr(nobs, ip))
        return n, slot, repl, nobs


    def search_by_sim3(self, other: "HostFrame", s12, pts1: dict, pts2: dict, matches_in=None, th=7.5):
        """ORBmatcher(0.75, true).SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (src/ORBmatcher.cc:1457-1674), this frame as keyframe 1
        and ``other`` as keyframe 2.  ``pts_k``: pos [n,3], desc [n,32], min_max [n,2], bad [n], slot [N_k] (point index per keypoint
        slot or -1).  Returns nFound and, per slot of keyframe 1, the matched keyframe-2 point index or -1."""
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        fp, ip, bp = capi.c_float_p, capi.c_int32_p, capi.c_uint8_p
        keep = [_f32(s12)]
        for p in (pts1, pts2):
            keep += [_f32(p["pos"]), u8(p["desc"]), _f32(p["min_max"]), u8(p["bad"]), _i32(p["slot"])]
        keep.append(_i32(matches_in if matches_in is not None else -np.ones(self.n)))
        out = -np.ones(self.n, dtype=np.int32)
        n = self.lib.osh_host_search_by_sim3(self.f, other.f, capi.ptr(keep[0], fp), float(th),
                                             len(pts1["pos"]), capi.ptr(keep[1], fp), capi.ptr(keep[2], bp), capi.ptr(keep[3], fp), capi.ptr(keep[4], bp), capi.ptr(keep[5], ip),
                                             len(pts2["pos"]), capi.ptr(keep[6], fp), capi.ptr(keep[7], bp), capi.ptr(keep[8], fp), capi.ptr(keep[9], bp), capi.ptr(keep[10], ip),
                                             capi.ptr(keep[11], ip), capi.ptr(out, ip))
        return n, out


def _quat_from_R(R):
    return synth._quat_from_R(np.asarray(R, dtype=np.float64))


class HostInertialGraph:
    """A map with IMU state built from a synth_inertial.LibaWindow: keyframe k <-> pose index k of the window
    (temporal keyframes ids 100+i, the fixed predecessor id 99, fixed observers ids 10+i)."""

    def __init__(self, w, no_prev=()):
        """``no_prev``: pose indices of temporal keyframes whose mPrevKF stays null (the chain of keyframes breaks before them;
        the window must not hold an inertial link that ends there)."""
        self.lib = capi.load_host_library()
        self.w = w
        assert not np.isin(w.link_cur, list(no_prev)).any()
        N, K = w.n_opt, w.n_opt + w.n_fixed_imu + w.n_fixed
        self.kf_id = np.array([100 + i for i in range(N)] + [99] * w.n_fixed_imu + [10 + i for i in range(w.n_fixed)], dtype=np.int64)
        self.mp_id = np.arange(w.n_points, dtype=np.int64) + 1000
        pose = np.zeros((K, 7), dtype=np.float32)
        for k in range(K):
            pose[k, :4] = _quat_from_R(w.pose_Rcw.reshape(-1, 3, 3)[k])
            pose[k, 4:] = w.pose_tcw.reshape(-1, 3)[k]
        cam5, inv = _f32(w.cam), _f32(synth.INV_LEVEL_SIGMA2)
        # a fisheye rig window: OSH_EDGE_RIGHT edges are right-camera observations, registered after the left ones (set_rig below)
        right = w.edge_kind == capi.OSH_EDGE_RIGHT
        left = ~right
        all_octave = _i32(np.round(np.log(1.0 / w.edge_info) / np.log(1.44)).astype(np.int32))
        octave = _i32(all_octave[left])
        obs, mp_pos = _f32(w.edge_obs[left]), _f32(w.points)
        self.g = C.c_void_p(self.lib.osh_host_graph_create(
            K, capi.ptr(self.kf_id, capi.c_int64_p), capi.ptr(pose, capi.c_float_p), capi.ptr(cam5, capi.c_float_p),
            capi.ptr(inv, capi.c_float_p), len(inv), w.n_points, capi.ptr(self.mp_id, capi.c_int64_p), capi.ptr(mp_pos, capi.c_float_p),
            int(left.sum()), capi.ptr(_i32(w.edge_pose[left]), capi.c_int32_p), capi.ptr(_i32(w.edge_point[left]), capi.c_int32_p),
            capi.ptr(obs, capi.c_float_p), capi.ptr(octave, capi.c_int32_p), -1 & 0x7FFFFFFF, 1))
        n_imu = N + w.n_fixed_imu
        kf_index = _i32(np.arange(n_imu))
        prev = _i32([-1 if i in no_prev else N if (i == 0 and w.n_fixed_imu) else i - 1 for i in range(N)] + [-1] * w.n_fixed_imu)
        vel = _f32(w.vel.reshape(-1, 3)[:n_imu])
        bias6 = _f32(np.concatenate([w.bias_a.reshape(-1, 3)[:n_imu], w.bias_g.reshape(-1, 3)[:n_imu]], axis=1))
        pre = np.zeros((n_imu, capi.OSH_PREINT_FLOATS), dtype=np.float32)
        cov = np.zeros((n_imu, 225), dtype=np.float32)
        for l in range(w.n_links):
            pre[int(w.link_cur[l])] = w.link_preint[l]
            cov[int(w.link_cur[l])] = w.gt["link_cov"][l].ravel()
        Tbc = w.gt["Tbc"]
        tbc_qt = _f32(np.concatenate([_quat_from_R(Tbc[:3, :3]), Tbc[:3, 3]]))
        self.lib.osh_host_graph_set_inertial(self.g, n_imu, capi.ptr(kf_index, capi.c_int32_p), capi.ptr(prev, capi.c_int32_p),
                                             capi.ptr(vel, capi.c_float_p), capi.ptr(bias6, capi.c_float_p), capi.ptr(pre, capi.c_float_p),
                                             capi.ptr(cov, capi.c_float_p), capi.ptr(tbc_qt, capi.c_float_p))
        if w.kb8 is not None:     # monocular fisheye map: every keyframe's mpCamera is one KannalaBrandt8
            self.lib.osh_host_graph_set_fisheye(self.g, capi.ptr(_f32(w.kb8), capi.c_float_p))
        if w.cam2 is not None:    # fisheye stereo rig: right camera, Trl and the right-camera observations
            r_uv = _f32(w.edge_obs[right][:, :2])
            rc = self.lib.osh_host_graph_set_rig(self.g, capi.ptr(_f32(w.cam2), capi.c_float_p), capi.ptr(_f32(w.gt["trl_qt"]), capi.c_float_p),
                                                 int(right.sum()), capi.ptr(_i32(w.edge_pose[right]), capi.c_int32_p),
                                                 capi.ptr(_i32(w.edge_point[right]), capi.c_int32_p), capi.ptr(r_uv, capi.c_float_p),
                                                 capi.ptr(_i32(all_octave[right]), capi.c_int32_p))
            assert rc == 0
        self.cur = N - 1

    def close(self):
        if self.g:
            self.lib.osh_host_graph_destroy(self.g)
            self.g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def packed_window(self, large=False, rec_init=False):
        """The osh_liba_problem the host layer builds, copied into a LibaWindow (for the oracle) + id maps."""
        from .synth_inertial import LibaWindow
        p = capi.LibaProblem()
        K = len(self.kf_id)
        kid, mid = np.zeros(K, dtype=np.int64), np.zeros(self.w.n_points, dtype=np.int64)
        rc = self.lib.osh_host_pack_liba(self.g, self.cur, int(large), int(rec_init), C.byref(p), capi.ptr(kid, capi.c_int64_p),
                                         capi.ptr(mid, capi.c_int64_p))
        assert rc == 0, rc

        w = self._window_of(p, lambda_init=1e-2 if large else 1.0, max_iterations=4 if large else 10)
        Kp = p.n_opt + p.n_fixed_imu + p.n_fixed
        return w, kid[:Kp], mid[:p.n_points]

    @staticmethod
    def _window_of(p, lambda_init, max_iterations):
        from .synth_inertial import LibaWindow

        def arr(ptr, n, dt=np.float64):
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dtype=dt)
        Kp, NV, L, E, NL = p.n_opt + p.n_fixed_imu + p.n_fixed, p.n_opt + p.n_fixed_imu, p.n_points, p.n_edges, p.n_links
        w = LibaWindow(
            n_opt=p.n_opt, n_fixed_imu=p.n_fixed_imu, n_fixed=p.n_fixed, pose_Rcw=arr(p.pose_Rcw, Kp * 9), pose_tcw=arr(p.pose_tcw, Kp * 3),
            pose_Rwb=arr(p.pose_Rwb, Kp * 9), pose_twb=arr(p.pose_twb, Kp * 3), Rcb=arr(p.Rcb, 9), tcb=arr(p.tcb, 3), tbc=arr(p.tbc, 3),
            cam=arr(p.cam, 5), vel=arr(p.vel, NV * 3), bias_g=arr(p.bias_g, NV * 3), bias_a=arr(p.bias_a, NV * 3),
            points=arr(p.points, L * 3).reshape(-1, 3), edge_pose=arr(p.edge_pose, E, np.int32), edge_point=arr(p.edge_point, E, np.int32),
            edge_kind=arr(p.edge_kind, E, np.uint8), edge_obs=arr(p.edge_obs, E * 3).reshape(-1, 3), edge_info=arr(p.edge_info, E),
            link_prev=arr(p.link_prev, NL, np.int32), link_cur=arr(p.link_cur, NL, np.int32),
            link_preint=arr(p.link_preint, NL * capi.OSH_PREINT_FLOATS, np.float32).reshape(NL, -1),
            link_info=arr(p.link_info, NL * 81).reshape(NL, 81), link_info_g=arr(p.link_info_g, NL * 9).reshape(NL, 9),
            link_info_a=arr(p.link_info_a, NL * 9).reshape(NL, 9), link_robust=arr(p.link_robust, NL, np.uint8),
            lambda_init=lambda_init, max_iterations=max_iterations,
            kb8=arr(p.kb8, 4) if p.kb8 else None, cam2=arr(p.cam2, 8) if p.cam2 else None, trl=arr(p.trl, 12) if p.trl else None,
            link_bias=arr(p.link_bias, NL, np.int32) if p.link_bias else None).normalise()
        return w

    def run(self, large=False, rec_init=False):
        return self.lib.osh_host_run_liba(self.g, self.cur, int(large), int(rec_init))

    def packed_full(self, its, fix_local=False, init=False, prior_g=1e2, prior_a=1e6):
        """The problem Optimizer::FullInertialBA(map, its, bFixLocal, ., ., bInit) solves, as (LibaWindow, keyframe ids, map point ids,
        number of keyframes no edge touches); the host layer's return code instead when it declines the case."""
        p = capi.LibaProblem()
        kid, mid = np.zeros(len(self.kf_id) + 1, dtype=np.int64), np.zeros(self.w.n_points, dtype=np.int64)
        idle = np.zeros(1, dtype=np.int32)
        rc = self.lib.osh_host_pack_full_inertial(self.g, int(its), int(fix_local), int(init), prior_g, prior_a, C.byref(p), capi.ptr(kid, capi.c_int64_p),
                                                  capi.ptr(mid, capi.c_int64_p), capi.ptr(idle, capi.c_int32_p))
        if rc != 0:
            return rc
        return self._window_of(p, 1e-5, int(its)), kid[:p.n_opt + p.n_fixed_imu + p.n_fixed], mid[:p.n_points], int(idle[0])

    def run_full(self, its, loop_id=0, fix_local=False, init=False, prior_g=1e2, prior_a=1e6):
        return self.lib.osh_host_run_full_inertial(self.g, int(its), int(fix_local), int(loop_id), int(init), prior_g, prior_a)

    def packed_merge(self, curr, merge):
        """The problem Optimizer::MergeInertialBA(kf[curr], kf[merge], ...) solves + (temporal keyframe ids, covisible keyframe ids) in
        the reference's order."""
        p = capi.LibaProblem()
        K = len(self.kf_id)
        kid, mid = np.zeros(K, dtype=np.int64), np.zeros(self.w.n_points, dtype=np.int64)
        sets, tid, cid = np.zeros(2, dtype=np.int32), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        rc = self.lib.osh_host_pack_merge_inertial(self.g, int(curr), int(merge), C.byref(p), capi.ptr(kid, capi.c_int64_p), capi.ptr(mid, capi.c_int64_p),
                                                   capi.ptr(sets, capi.c_int32_p), capi.ptr(tid, capi.c_int64_p), capi.ptr(cid, capi.c_int64_p))
        if rc != 0:
            return rc
        return (self._window_of(p, 1e3, 8), kid[:p.n_opt + p.n_fixed_imu + p.n_fixed], mid[:p.n_points], tid[:sets[0]], cid[:sets[1]])

    def run_merge(self, curr, merge):
        """Optimizer::MergeInertialBA; returns corrPoses as {keyframe id: [qx qy qz qw tx ty tz s]}."""
        K = len(self.kf_id)
        ids, sim = np.zeros(K, dtype=np.int64), np.zeros((K, 8))
        n = self.lib.osh_host_run_merge_inertial(self.g, int(curr), int(merge), K, capi.ptr(ids, capi.c_int64_p), capi.ptr(sim, capi.c_double_p))
        assert 0 <= n <= K, n
        return {int(ids[i]): sim[i].copy() for i in range(n)}

    def kf_inertial_gba(self, i):
        """(mnBAGlobalForKF, mTcwGBA [qx qy qz qw tx ty tz], mVwbGBA, mBiasGBA [ba, bg]) of keyframe i."""
        pose, vel, bias = np.zeros(7, dtype=np.float32), np.zeros(3, dtype=np.float32), np.zeros(6, dtype=np.float32)
        self.lib.osh_host_get_kf_pose_gba(self.g, i, capi.ptr(pose, capi.c_float_p))
        lid = self.lib.osh_host_get_kf_inertial_gba(self.g, i, capi.ptr(vel, capi.c_float_p), capi.ptr(bias, capi.c_float_p))
        return int(lid), pose, vel, bias

    def kf_pose(self, i):
        o = np.zeros(7, dtype=np.float32)
        self.lib.osh_host_get_kf_pose(self.g, i, capi.ptr(o, capi.c_float_p))
        return o

    def kf_velocity(self, i):
        o = np.zeros(3, dtype=np.float32)
        self.lib.osh_host_get_kf_velocity(self.g, i, capi.ptr(o, capi.c_float_p))
        return o

    def kf_bias(self, i):
        o = np.zeros(6, dtype=np.float32)
        self.lib.osh_host_get_kf_bias(self.g, i, capi.ptr(o, capi.c_float_p))
        return o

    def mp_pos(self, j):
        o = np.zeros(3, dtype=np.float32)
        self.lib.osh_host_get_mp_pos(self.g, j, capi.ptr(o, capi.c_float_p))
        return o


def host_preintegrate(acc, gyr, dt, bias6, nga6, walk6):
    lib = capi.load_host_library()
    acc, gyr = _f32(acc), _f32(gyr)
    rec, cov = np.zeros(capi.OSH_PREINT_FLOATS, dtype=np.float32), np.zeros(225, dtype=np.float32)
    fp = capi.c_float_p
    lib.osh_host_preintegrate(len(acc), capi.ptr(acc, fp), capi.ptr(gyr, fp), np.float32(dt), capi.ptr(_f32(bias6), fp),
                              capi.ptr(_f32(nga6), fp), capi.ptr(_f32(walk6), fp), capi.ptr(rec, fp), capi.ptr(cov, fp))
    return rec, cov.reshape(15, 15)


def host_inertial_information(cov):
    lib = capi.load_host_library()
    out = np.zeros(81)
    lib.osh_host_inertial_information(capi.ptr(_f32(cov).ravel(), capi.c_float_p), capi.ptr(out, capi.c_double_p))
    return out.reshape(9, 9)


class HostPoseiFrame:
    """A tracked frame + its IMU link built from a synth_inertial.PoseiFrame, for Optimizer::PoseInertialOptimizationLastKeyFrame
    (mode 0) / LastFrame (mode 1) through the reference signatures.  Keypoint k <-> edge order[k] of the flat frame (a fisheye rig
    frame lists its left keypoints first)."""

    def __init__(self, f):
        self.lib = capi.load_host_library()
        self.f = f
        right = f.edge_kind == capi.OSH_EDGE_RIGHT
        rig = f.cam2 is not None
        self.order = np.concatenate([np.nonzero(~right)[0], np.nonzero(right)[0]]) if rig else np.arange(f.n_edges)
        o = self.order
        n_left = int((~right).sum()) if rig else -1
        Tbc = np.eye(4)
        Tbc[:3, :3], Tbc[:3, 3] = f.Rcb.reshape(3, 3).T, f.tbc
        tbc_qt = _f32(np.concatenate([_quat_from_R(Tbc[:3, :3]), Tbc[:3, 3]]))

        def tcw_qt(Rwb, twb):      # Tcw = Tcb * Tbw
            Rcb = f.Rcb.reshape(3, 3)
            Rcw = Rcb @ Rwb.reshape(3, 3).T
            return _f32(np.concatenate([_quat_from_R(Rcw), Rcb @ (-Rwb.reshape(3, 3).T @ twb) + f.tcb]))
        pose = _f32(np.concatenate([_quat_from_R(f.Rcw.reshape(3, 3)), f.tcw]))
        prev_pose = tcw_qt(f.prev_Rwb, f.prev_twb)
        octave = _i32(np.round(np.log(1.0 / f.edge_info[o]) / np.log(1.44)).astype(np.int32))
        uright = _f32(np.where(f.edge_kind[o] == capi.OSH_EDGE_STEREO, f.edge_obs[o, 2], -1.0))
        cov = np.zeros((15, 15), dtype=np.float32)
        cov[:9, :9] = np.linalg.inv(f.info_inertial.reshape(9, 9))
        cov[9:12, 9:12] = np.linalg.inv(f.info_g.reshape(3, 3))
        cov[12:15, 12:15] = np.linalg.inv(f.info_a.reshape(3, 3))
        fp = lambda a: capi.ptr(_f32(a), capi.c_float_p) if a is not None else None   # noqa: E731
        dp = lambda a: capi.ptr(np.ascontiguousarray(a, dtype=np.float64), capi.c_double_p) if a is not None else None   # noqa: E731
        self._keep = [pose, prev_pose, octave, uright, tbc_qt, cov]
        self.h = C.c_void_p(self.lib.osh_host_posei_create(
            int(f.mode), f.n_edges, fp(f.edge_obs[o, :2]), capi.ptr(octave, capi.c_int32_p), capi.ptr(uright, capi.c_float_p), n_left,
            capi.ptr(pose, capi.c_float_p), fp(f.cam), fp(f.kb8), fp(f.cam2), fp(f.gt["trl_qt"]) if rig else None, fp(synth.INV_LEVEL_SIGMA2),
            len(synth.INV_LEVEL_SIGMA2), fp(f.points[o]), capi.ptr(np.ascontiguousarray(f.edge_close[o]), capi.c_uint8_p),
            capi.ptr(tbc_qt, capi.c_float_p), fp(f.vel), fp(np.concatenate([f.bias_a, f.bias_g])), capi.ptr(prev_pose, capi.c_float_p), fp(f.prev_vel),
            fp(np.concatenate([f.prev_bias_a, f.prev_bias_g])), capi.ptr(np.ascontiguousarray(f.preint), capi.c_float_p),
            capi.ptr(np.ascontiguousarray(cov.ravel()), capi.c_float_p), dp(f.prior_Rwb), dp(f.prior_twb), dp(f.prior_vel), dp(f.prior_bg), dp(f.prior_ba),
            dp(f.prior_H)))
        assert self.h

    def close(self):
        if self.h:
            self.lib.osh_host_posei_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def packed(self, rec_init=False):
        """The osh_posei_problem the host layer builds, copied into a PoseiFrame (for the oracle) + the keypoint of every edge."""
        from .synth_inertial import PoseiFrame
        p = capi.PoseiProblem()
        kp = np.zeros(self.f.n_edges, dtype=np.int32)
        rc = self.lib.osh_host_posei_pack(self.h, int(rec_init), C.byref(p), capi.ptr(kp, capi.c_int32_p))
        assert rc == 0, rc

        def arr(ptr, n, dt=np.float64):
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy() if ptr else None
        E = p.n_edges
        g = PoseiFrame(
            mode=p.mode, Rcw=arr(p.Rcw, 9), tcw=arr(p.tcw, 3), Rwb=arr(p.Rwb, 9), twb=arr(p.twb, 3), vel=arr(p.vel, 3), bias_g=arr(p.bias_g, 3),
            bias_a=arr(p.bias_a, 3), prev_Rwb=arr(p.prev_Rwb, 9), prev_twb=arr(p.prev_twb, 3), prev_vel=arr(p.prev_vel, 3),
            prev_bias_g=arr(p.prev_bias_g, 3), prev_bias_a=arr(p.prev_bias_a, 3), Rcb=arr(p.Rcb, 9), tcb=arr(p.tcb, 3), tbc=arr(p.tbc, 3), cam=arr(p.cam, 5),
            preint=arr(p.preint, capi.OSH_PREINT_FLOATS, np.float32), info_inertial=arr(p.info_inertial, 81), info_g=arr(p.info_g, 9), info_a=arr(p.info_a, 9),
            points=arr(p.points, E * 3).reshape(-1, 3), edge_kind=arr(p.edge_kind, E, np.uint8), edge_obs=arr(p.edge_obs, E * 3).reshape(-1, 3),
            edge_info=arr(p.edge_info, E), edge_close=arr(p.edge_close, E, np.uint8), prior_Rwb=arr(p.prior_Rwb, 9), prior_twb=arr(p.prior_twb, 3),
            prior_vel=arr(p.prior_vel, 3), prior_bg=arr(p.prior_bg, 3), prior_ba=arr(p.prior_ba, 3), prior_H=arr(p.prior_H, 225), kb8=arr(p.kb8, 4),
            cam2=arr(p.cam2, 8), trl=arr(p.trl, 12), rec_init=bool(p.rec_init), huber_mono=p.huber_mono, huber_stereo=p.huber_stereo, huber_prior=p.huber_prior,
            chi2_mono=tuple(p.chi2_mono), chi2_stereo=tuple(p.chi2_stereo), iterations=tuple(p.iterations)).normalise()
        return g, kp[:E]

    def run(self, rec_init=False):
        pose, Rwb, twb, vel, bias = (np.zeros(k, dtype=np.float32) for k in (7, 9, 3, 3, 6))
        outlier = np.zeros(self.f.n_edges, dtype=np.uint8)
        H = np.zeros(225)
        gone = C.c_int32(0)
        n = self.lib.osh_host_posei_run(self.h, int(rec_init), capi.ptr(pose, capi.c_float_p), capi.ptr(Rwb, capi.c_float_p), capi.ptr(twb, capi.c_float_p),
                                        capi.ptr(vel, capi.c_float_p), capi.ptr(bias, capi.c_float_p), capi.ptr(outlier, capi.c_uint8_p),
                                        capi.ptr(H, capi.c_double_p), C.byref(gone))
        return dict(n=n, pose_qt=pose, Rwb=Rwb.reshape(3, 3), twb=twb, vel=vel, bias_a=bias[:3], bias_g=bias[3:], outlier=outlier, H=H.reshape(15, 15),
                    prev_cpi_deleted=bool(gone.value))


def search_by_bow_keyframes(desc1, angle1, has_mp1, fv1, desc2, angle2, has_mp2, fv2, nnratio=0.7, check_ori=True):
    """ORBmatcher(nnratio, check_ori).SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:765-905) on two keyframes built from flat
    features; returns (nmatches, match12[n1]) with match12[i] = feature of keyframe 2 whose map point was matched to feature i."""
    lib = capi.load_host_library()
    d1, d2 = np.ascontiguousarray(desc1, dtype=np.uint8), np.ascontiguousarray(desc2, dtype=np.uint8)
    keep = [d1, _f32(angle1), np.ascontiguousarray(has_mp1, dtype=np.uint8)] + [_i32(a) for a in fv1] + \
           [d2, _f32(angle2), np.ascontiguousarray(has_mp2, dtype=np.uint8)] + [_i32(a) for a in fv2]
    m = np.zeros(len(d1), dtype=np.int32)
    n = lib.osh_host_search_by_bow_kf(len(d1), capi.ptr(keep[0], capi.c_uint8_p), capi.ptr(keep[1], capi.c_float_p), capi.ptr(keep[2], capi.c_uint8_p),
                                      len(keep[3]), capi.ptr(keep[3], capi.c_int32_p), capi.ptr(keep[4], capi.c_int32_p), capi.ptr(keep[5], capi.c_int32_p),
                                      len(d2), capi.ptr(keep[6], capi.c_uint8_p), capi.ptr(keep[7], capi.c_float_p), capi.ptr(keep[8], capi.c_uint8_p),
                                      len(keep[9]), capi.ptr(keep[9], capi.c_int32_p), capi.ptr(keep[10], capi.c_int32_p), capi.ptr(keep[11], capi.c_int32_p),
                                      float(nnratio), int(check_ori), capi.ptr(m, capi.c_int32_p))
    return n, m


def search_for_triangulation(kp1, octave1, desc1, has_mp1, pose1_qt, fv1, kp2, octave2, desc2, has_mp2, pose2_qt, fv2, only_stereo=False, coarse=False,
                             check_ori=True):
    """ORBmatcher(0.6, check_ori).SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:907-1146) on
    two pinhole keyframes built from flat features (kp = x, y, angle, uright); returns (nmatches, match12[n1])."""
    lib = capi.load_host_library()
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    cam4 = _f32([synth.FX, synth.FY, synth.CX, synth.CY])
    keep = [cam4, _f32(kp1), _i32(octave1), u8(desc1), u8(has_mp1), _f32(pose1_qt)] + [_i32(a) for a in fv1] + \
           [_f32(kp2), _i32(octave2), u8(desc2), u8(has_mp2), _f32(pose2_qt)] + [_i32(a) for a in fv2]
    m = -np.ones(len(octave1), dtype=np.int32)
    fp, ip, bp = capi.c_float_p, capi.c_int32_p, capi.c_uint8_p
    n = lib.osh_host_search_for_triangulation(capi.ptr(keep[0], fp), int(synth.N_LEVELS), float(synth.SCALE_FACTOR), len(octave1), capi.ptr(keep[1], fp),
                                              capi.ptr(keep[2], ip), capi.ptr(keep[3], bp), capi.ptr(keep[4], bp), capi.ptr(keep[5], fp), len(keep[6]),
                                              capi.ptr(keep[6], ip), capi.ptr(keep[7], ip), capi.ptr(keep[8], ip), len(octave2), capi.ptr(keep[9], fp),
                                              capi.ptr(keep[10], ip), capi.ptr(keep[11], bp), capi.ptr(keep[12], bp), capi.ptr(keep[13], fp), len(keep[14]),
                                              capi.ptr(keep[14], ip), capi.ptr(keep[15], ip), capi.ptr(keep[16], ip), int(only_stereo), int(coarse),
                                              int(check_ori), capi.ptr(m, ip))
    return n, m


def search_for_initialization(f1, f2, prev_xy, window=100, nnratio=0.9, check_ori=True):
    """ORBmatcher(nnratio, check_ori).SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:648-763)
    on two HostFrames; returns (nmatches, vnMatches12, the updated vbPrevMatched)."""
    lib = capi.load_host_library()
    prev = np.array(prev_xy, dtype=np.float32)
    m = -np.ones(f1.n, dtype=np.int32)
    n = lib.osh_host_search_for_initialization(f1.f, f2.f, capi.ptr(prev, capi.c_float_p), int(window), float(nnratio), int(check_ori),
                                               capi.ptr(m, capi.c_int32_p))
    return n, m, prev


def _bow_result(o: dict) -> "capi.BowResult":
    from . import orb
    r = capi.BowResult()
    orb._wire_outputs(r, o)
    return r


def bow_restatement(tree, desc, levelsup: int = 4, timed: bool = False):
    """osh_host_bow_restatement: TemplatedVocabulary::transform restated in one C++ thread on a synth_bow.BowTree and descriptors
    [n, 32]; the dict of orb.OrbMatcher.bow_transform(.., stages=True) (with `timed`: that and the milliseconds)."""
    from . import orb
    lib = capi.load_host_library()
    t, _keep = orb.bow_tree(tree)
    d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
    o = orb.bow_outputs(d.shape[0], stages=True)
    ms = C.c_double(0)
    rc = lib.osh_host_bow_restatement(C.byref(t), int(levelsup), d.shape[0], capi.ptr(d, capi.c_uint8_p), C.byref(_bow_result(o)), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_bow_restatement returned {rc}")
    return (orb.bow_trim(o), float(ms.value)) if timed else orb.bow_trim(o)


class HostBowVocab:
    """An ORB_SLAM3::ORBVocabulary loaded from a text file (osh_host_bow_vocab_load); `loaded` is what loadFromTextFile returned."""

    def __init__(self, path):
        self.lib = capi.load_host_library()
        self.h = self.lib.osh_host_bow_vocab_load(str(path).encode())
        self.loaded = bool(self.h)

    def close(self):
        if self.h:
            self.lib.osh_host_bow_vocab_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def tree(self, levelsup: int = 4):
        """(synth_bow.BowTree of the loaded arrays, dict of the getters, getParentNode(w, levelsup) of every word)."""
        from . import synth_bow
        info = np.zeros(7, dtype=np.int32)
        ip = capi.ptr(info, capi.c_int32_p)
        assert self.lib.osh_host_bow_vocab_tree(self.h, ip, None, None, None, None, 0, None) == 0
        n, words = int(info[4]), int(info[5])
        parent, leaf, desc = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
        weight, word_parent = np.zeros(n, np.float64), np.zeros(words, np.int32)
        assert self.lib.osh_host_bow_vocab_tree(self.h, ip, capi.ptr(parent, capi.c_int32_p), capi.ptr(leaf, capi.c_uint8_p),
                                                capi.ptr(desc, capi.c_uint8_p), capi.ptr(weight, capi.c_double_p), int(levelsup),
                                                capi.ptr(word_parent, capi.c_int32_p)) == 0
        k, L, weighting, scoring = (int(x) for x in info[:4])
        getters = dict(k=k, L=L, weighting=weighting, scoring=scoring, size=words, empty=bool(info[6]))
        return synth_bow.BowTree(k, L, weighting, scoring, parent, leaf, desc, weight), getters, word_parent

    def compute_bow(self, desc, keyframe: bool = False, second_desc=None, n_threads: int = 1) -> dict:
        """Frame::ComputeBoW (or KeyFrame::ComputeBoW) on a stand-in with these descriptors: mBowVec as word_id / word_value and
        mFeatVec as node_id / node_start / node_feat.  second_desc: ComputeBoW is called once more after the descriptors were
        replaced by it.  n_threads > 1: as many threads do the same at once and have to agree."""
        from . import orb
        d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        d2 = None if second_desc is None else np.ascontiguousarray(second_desc, dtype=np.uint8).reshape(-1, 32)
        assert d2 is None or d2.shape == d.shape
        o = orb.bow_outputs(d.shape[0], stages=False)
        rc = self.lib.osh_host_bow_compute(self.h, int(keyframe), d.shape[0], capi.ptr(d, capi.c_uint8_p), capi.ptr(d2, capi.c_uint8_p),
                                           int(n_threads), C.byref(_bow_result(o)))
        if rc != 0:
            raise RuntimeError(f"osh_host_bow_compute returned {rc}")
        return orb.bow_trim(o)


def bow_score(id1, value1, id2, value2) -> float:
    """ORBVocabulary::score (L1) of two BowVectors given as word ids and values."""
    lib = capi.load_host_library()
    a = [_i32(id1), np.ascontiguousarray(value1, np.float64), _i32(id2), np.ascontiguousarray(value2, np.float64)]
    return float(lib.osh_host_bow_score(len(a[0]), capi.ptr(a[0], capi.c_int32_p), capi.ptr(a[1], capi.c_double_p),
                                        len(a[2]), capi.ptr(a[2], capi.c_int32_p), capi.ptr(a[3], capi.c_double_p)))


def _kfdb_graph(g):
    """capi.HostKfdbGraph of a synth_kfdb.KfdbGraph and the arrays its pointers refer to."""
    def csr(lists, dtype=np.int32):
        start = np.zeros(len(lists) + 1, np.int32)
        start[1:] = np.cumsum([len(x) for x in lists])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype) for x in lists] + [np.zeros(0, dtype)]), dtype)
        return start, flat
    a = dict(kf_id=_i32(g.kf_id), kf_map=_i32(g.kf_map), kf_bad=np.ascontiguousarray(g.kf_bad, np.uint8),
             map_bad=np.ascontiguousarray(g.map_bad, np.uint8), fr_id=_i32([f[0] for f in g.frames]))
    a["bow_start"], a["bow_word"] = csr([b[0] for b in g.bow])
    _, a["bow_value"] = csr([b[1] for b in g.bow], np.float64)
    a["cov_start"], a["cov"] = csr(g.cov)
    a["con_start"], a["con"] = csr(g.con)
    a["fr_start"], a["fr_word"] = csr([f[1] for f in g.frames])
    _, a["fr_value"] = csr([f[2] for f in g.frames], np.float64)
    c = capi.HostKfdbGraph()
    c.n_words, c.n_kf, c.n_maps, c.n_frames = int(g.n_words), g.n_kf, len(g.map_bad), len(g.frames)
    for name, arr in a.items():
        typ = {np.dtype(np.int32): capi.c_int32_p, np.dtype(np.uint8): capi.c_uint8_p, np.dtype(np.float64): capi.c_double_p}[arr.dtype]
        setattr(c, name, capi.ptr(arr, typ))
    return c, a


def _kfdb_script(symbol, handle, g, ops):
    """Runs a script of (code, a, b) operations; per query a dict with loop / merge (keyframe indices), marker [n_kf, 4] and
    score [n_kf, 2] (see osh_host_kfdb_out), and the wall time of the queries in ms."""
    lib = capi.load_host_library()
    c, _keep = _kfdb_graph(g)
    ops = np.ascontiguousarray(ops, np.int32).reshape(-1, 3)
    nq = max(int(np.sum(ops[:, 0] >= 4)), 1)
    n = max(g.n_kf, 1)
    o = dict(n_loop=np.zeros(nq, np.int32), loop=np.zeros((nq, n), np.int32), n_merge=np.zeros(nq, np.int32), merge=np.zeros((nq, n), np.int32),
             marker=np.zeros((nq, n, 4), np.int64), score=np.zeros((nq, n, 2), np.float32))
    out = capi.HostKfdbOut()
    for name, arr in o.items():
        typ = {np.dtype(np.int32): capi.c_int32_p, np.dtype(np.int64): capi.c_int64_p, np.dtype(np.float32): capi.c_float_p}[arr.dtype]
        setattr(out, name, capi.ptr(arr, typ))
    ms = C.c_double(0)
    args = (C.byref(c), ops.shape[0], capi.ptr(ops, capi.c_int32_p), C.byref(out), C.byref(ms))
    rc = getattr(lib, symbol)(*(args if handle is None else (handle,) + args))
    if rc < 0:
        raise RuntimeError(f"{symbol} returned {rc}")
    res = [dict(loop=o["loop"][q, :o["n_loop"][q]].tolist(), merge=o["merge"][q, :o["n_merge"][q]].tolist(),
                marker=o["marker"][q, :g.n_kf].copy(), score=o["score"][q, :g.n_kf].copy()) for q in range(rc)]
    return res, float(ms.value)


def kfdb_restatement(g, ops):
    """The script on the single-thread C++ restatement of the reference's KeyFrameDatabase (osh_host_kfdb_restatement)."""
    return _kfdb_script("osh_host_kfdb_restatement", None, g, ops)


def kfdb_run(voc: "HostBowVocab", g, ops):
    """The script on an ORB_SLAM3::KeyFrameDatabase over the loaded vocabulary (osh_host_kfdb_run)."""
    return _kfdb_script("osh_host_kfdb_run", voc.h, g, ops)


def bowdb_check_words(word_id, n_words: int) -> int:
    """bowdb_check_words of csrc/bowdb_book.h: 0 accepted, 1 not ascending or a duplicate, 2 an id outside the vocabulary."""
    w = _i32(word_id)
    return int(capi.load_host_library().osh_host_bowdb_check_words(len(w), capi.ptr(w, capi.c_int32_p), int(n_words)))


def bowdb_book_replay(ops, max_rows: int = 1 << 16) -> dict:
    """A script of (0, entries) adds, (1, handle) erases and (2, 0) clears through the bookkeeping of osh_bow_db, without a device:
    op_handle per operation, the row table (handle, start, len, alive) and info (osh_host_bowdb_book_replay)."""
    lib = capi.load_host_library()
    ops = np.ascontiguousarray(ops, np.int64).reshape(-1, 2)
    u64 = C.POINTER(C.c_uint64)
    o = dict(op_handle=np.zeros(max(len(ops), 1), np.uint64), handle=np.zeros(max_rows, np.uint64), start=np.zeros(max_rows, np.int64),
             len=np.zeros(max_rows, np.int32), alive=np.zeros(max_rows, np.uint8), info=np.zeros(8, np.int64))
    rc = lib.osh_host_bowdb_book_replay(len(ops), capi.ptr(ops, capi.c_int64_p), capi.ptr(o["op_handle"], u64), max_rows, capi.ptr(o["handle"], u64),
                                        capi.ptr(o["start"], capi.c_int64_p), capi.ptr(o["len"], capi.c_int32_p),
                                        capi.ptr(o["alive"], capi.c_uint8_p), capi.ptr(o["info"], capi.c_int64_p))
    if rc < 0:
        raise RuntimeError(f"osh_host_bowdb_book_replay returned {rc}")
    names = ("live_rows", "rows", "entries", "capacity", "compactions", "reallocations", "row_capacity", "moved")
    return dict(op_handle=o["op_handle"][:len(ops)], handle=o["handle"][:rc], start=o["start"][:rc], len=o["len"][:rc], alive=o["alive"][:rc],
                info=dict(zip(names, (int(x) for x in o["info"]))))


def newpoint_triangulate_cpu(segments):
    """csrc/newpoint_triangulate.h on the host in one thread (osh_host_newpoint_triangulate_cpu): per-segment output dicts, ms."""
    from . import orb
    return orb.newpoint_cpu(segments)


def two_view_reconstruct(scene, camera: str = "class", iterations: int = 200, p3d_in=None) -> dict:
    """TwoViewReconstruction::Reconstruct (camera "class": K, sigma and `iterations` of the scene), Pinhole::ReconstructWithTwoViews
    ("pinhole") or KannalaBrandt8::ReconstructWithTwoViews ("kb8", the scene's fisheye parameters) on a synth_two_view.Scene
    (osh_host_two_view_reconstruct); the two cameras run the class defaults, 200 iterations.  p3d_in: what vP3D holds on entry
    [m, 3], m <= n1.  Returns ok, T21 [12], p3d [n1, 3] and triangulated [n1] (the first n_p3d / n_triangulated entries are what
    Reconstruct left), sets [iterations, 8] and info = (status, 1 if the device answered, mvSets.size())."""
    lib = capi.load_host_library()
    kind = {"class": 0, "pinhole": 1, "kb8": 2}[camera]
    K = np.asarray(scene.K, np.float32)
    params = {0: K.reshape(9), 1: np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32), 2: scene.kb8}[kind]
    params = np.ascontiguousarray(params, np.float32)
    if kind:
        iterations = 200
    xy1, xy2 = np.ascontiguousarray(scene.keys1, np.float32), np.ascontiguousarray(scene.keys2, np.float32)
    m12 = np.ascontiguousarray(scene.matches12, np.int32)
    n1 = xy1.shape[0]
    p3d = np.zeros((n1, 3), np.float32)
    n_p3d = C.c_int32(0)
    if p3d_in is not None:
        p3d_in = np.asarray(p3d_in, np.float32).reshape(-1, 3)
        p3d[:p3d_in.shape[0]] = p3d_in
        n_p3d = C.c_int32(p3d_in.shape[0])
    tri, n_tri = np.zeros(n1, np.uint8), C.c_int32(0)
    T21, sets, info = np.zeros(12, np.float32), np.zeros((iterations, 8), np.int32), np.zeros(3, np.int32)
    rc = lib.osh_host_two_view_reconstruct(kind, capi.ptr(params, capi.c_float_p), float(scene.sigma), iterations, n1, capi.ptr(xy1, capi.c_float_p),
                                           xy2.shape[0], capi.ptr(xy2, capi.c_float_p), capi.ptr(m12, capi.c_int32_p), capi.ptr(T21, capi.c_float_p),
                                           capi.ptr(p3d, capi.c_float_p), C.byref(n_p3d), capi.ptr(tri, capi.c_uint8_p), C.byref(n_tri),
                                           capi.ptr(sets, capi.c_int32_p), capi.ptr(info, capi.c_int32_p))
    if rc < 0:
        raise RuntimeError(f"osh_host_two_view_reconstruct returned {rc}")
    return dict(ok=bool(rc), T21=T21, p3d=p3d, n_p3d=int(n_p3d.value), triangulated=tri, n_triangulated=int(n_tri.value), sets=sets, info=info)


class MlpnpSolver:
    """An MLPnPsolver (include/MLPnPsolver.h) of the stand-in classes, built from a synth_mlpnp.Problem: keypoint i of the frame is
    correspondence order[i] (default: the problem's order), with `extra` keypoints without a map point in front and `bad` bad map
    points behind; level_sigma2 is 1.2^(2 l) and every keypoint's octave is the one its max_error came from.  relocalisation: the
    parameters Tracking::Relocalization sets (0.99, 10, 300, 6, 0.5, 5.991) instead of the constructor's."""

    def __init__(self, pb, extra: int = 0, bad: int = 0, relocalisation: bool = False, ransac=None):
        self.lib = capi.load_host_library()
        n = pb.n
        self.n_matches = extra + n + bad
        self.index = extra + np.arange(n)     # mvKeyPointIndices of the problem's correspondences
        sigma2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
        octave = np.zeros(self.n_matches, np.int32)
        octave[self.index] = np.argmin(np.abs(np.asarray(pb.max_error, np.float32)[:, None] / np.float32(5.991) - sigma2[None, :]), 1)
        xy = np.zeros((self.n_matches, 2), np.float32)
        xy[self.index] = pb.p2d
        world = np.zeros((self.n_matches, 3), np.float32)
        world[self.index] = pb.p3d
        state = np.zeros(self.n_matches, np.uint8)
        state[self.index] = 1
        state[extra + n:] = 2
        cam = np.ascontiguousarray(pb.camera, np.float32)
        self.handle = self.lib.osh_host_mlpnp_solver_create(int(pb.camera_type), capi.ptr(cam, capi.c_float_p), self.n_matches, capi.ptr(xy, capi.c_float_p),
                                                            capi.ptr(octave, capi.c_int32_p), 8, capi.ptr(sigma2, capi.c_float_p), self.n_matches,
                                                            capi.ptr(world, capi.c_float_p), capi.ptr(state, capi.c_uint8_p))
        if not self.handle:
            raise RuntimeError("osh_host_mlpnp_solver_create refused the arguments")
        if relocalisation:
            ransac = (0.99, 10, 300, 6, 0.5, 5.991)
        if ransac is not None:
            self.set_ransac(*ransac)

    def set_ransac(self, probability, min_inliers, max_iterations, min_set, epsilon, th2):
        if self.lib.osh_host_mlpnp_solver_set_ransac(self.handle, probability, min_inliers, max_iterations, min_set, epsilon, th2) != 0:
            raise RuntimeError("osh_host_mlpnp_solver_set_ransac")

    def state(self) -> dict:
        out = np.zeros(7, np.int32)
        self.lib.osh_host_mlpnp_solver_state(self.handle, capi.ptr(out, capi.c_int32_p))
        return dict(zip(("N", "min_inliers", "max_iterations", "iterations", "best_inliers", "queued_sets", "on_device"), (int(v) for v in out)))

    def iterate(self, n_iterations: int) -> dict:
        return mlpnp_iterate([self], n_iterations, batch=False)[0]

    def prepare(self, n_iterations: int, capacity: int = 1024):
        """The sets one iterate(n_iterations) would run: [count, 6] (None when N < mRansacMinInliers)."""
        sets = np.zeros((capacity, 6), np.int32)
        rc = self.lib.osh_host_mlpnp_solver_prepare(self.handle, n_iterations, capacity, capi.ptr(sets, capi.c_int32_p))
        if rc == -2:
            return None
        if rc < 0:
            raise RuntimeError(f"osh_host_mlpnp_solver_prepare -> {rc}")
        return sets[:min(rc, capacity)], rc

    def replay(self, first_hit=-1, hit_record=-1, hit_count=0, best_iteration=-1, best_count=0, best_refine_ok=0, hit_pose=None, hit_flags=None,
               best_pose=None, best_flags=None) -> dict:
        """Walks a given answer of the device for the prepared round as iterate would."""
        n = self.state()["N"]
        words = capi.ransac_mask_words(n)

        def mask(flags):
            bits = np.zeros(words * 32, np.uint8)
            if flags is not None:
                bits[:n] = np.asarray(flags, bool)
            return np.packbits(bits, bitorder="little").view(np.uint32).copy()

        head = np.array([first_hit, hit_record, hit_count, best_iteration, best_count, best_refine_ok], np.int32)
        hp = np.ascontiguousarray(np.zeros(12) if hit_pose is None else hit_pose, np.float64)
        bp = np.ascontiguousarray(np.zeros(12) if best_pose is None else best_pose, np.float64)
        hm, bm = mask(hit_flags), mask(best_flags)
        no_more, n_in = np.zeros(1, np.uint8), np.zeros(1, np.int32)
        inl, T = np.zeros(self.n_matches + 1, np.uint8), np.zeros(16, np.float32)
        rc = self.lib.osh_host_mlpnp_solver_replay(self.handle, capi.ptr(head, capi.c_int32_p), capi.ptr(hp, capi.c_double_p), capi.ptr(hm, capi.c_uint32_p),
                                                   capi.ptr(bp, capi.c_double_p), capi.ptr(bm, capi.c_uint32_p), self.n_matches,
                                                   capi.ptr(no_more, capi.c_uint8_p), capi.ptr(n_in, capi.c_int32_p), capi.ptr(inl, capi.c_uint8_p),
                                                   capi.ptr(T, capi.c_float_p))
        if rc < 0:
            raise RuntimeError(f"osh_host_mlpnp_solver_replay -> {rc}")
        return dict(found=bool(rc), no_more=bool(no_more[0]), n_inliers=int(n_in[0]), inliers=inl[:-1].astype(bool), has_inliers=bool(inl[-1]),
                    Tout=T.reshape(4, 4))

    def close(self):
        if self.handle:
            self.lib.osh_host_mlpnp_solver_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def mlpnp_iterate(solvers, n_iterations: int, batch: bool = True) -> list:
    """iterate(n_iterations, ..) of every MlpnpSolver, through MLPnPsolver::IterateBatch (one device call) or one by one: per solver
    a dict with found, no_more, n_inliers, inliers [n_matches], has_inliers (vbInliers not empty) and Tout [4, 4]."""
    lib = capi.load_host_library()
    S = len(solvers)
    m = max([s.n_matches for s in solvers], default=0)
    handles = (C.c_void_p * max(S, 1))(*[s.handle for s in solvers])
    found, no_more, n_in = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros(S, np.int32)
    inl, T = np.zeros((S, m + 1), np.uint8), np.zeros((S, 16), np.float32)
    rc = lib.osh_host_mlpnp_solver_iterate(S, handles, int(n_iterations), int(batch), m, capi.ptr(found, capi.c_uint8_p), capi.ptr(no_more, capi.c_uint8_p),
                                           capi.ptr(n_in, capi.c_int32_p), capi.ptr(inl, capi.c_uint8_p), capi.ptr(T, capi.c_float_p))
    if rc != 0:
        raise RuntimeError(f"osh_host_mlpnp_solver_iterate -> {rc}")
    return [dict(found=bool(found[k]), no_more=bool(no_more[k]), n_inliers=int(n_in[k]), inliers=inl[k, :s.n_matches].astype(bool),
                 has_inliers=bool(inl[k, m]), Tout=T[k].reshape(4, 4).copy()) for k, s in enumerate(solvers)]


class Sim3Scene:
    """What a Sim3Solver's constructor reads, as flat arrays (osh_host_sim3_scene), built from a synth_sim3_ransac.Problem:
    correspondence i is slot slot[i] of pKF1 (n1 slots in all), its map point of map 1 is point i and sits at keypoint key1[i] of
    pKF1, its map point of map 2 is point n + i and sits at keypoint key2[i] of pKF2.  The keyword sets name correspondences that
    are spoilt: null_match (vpMatched12 entry NULL), null_kf1 (pKF1's slot empty), bad1 / bad2 (a bad point), unindexed1 /
    unindexed2 (the point does not observe its keyframe), other_kf (the second point is observed in a third keyframe only).
    matched_kf: None passes vpKeyFrameMatchedMP empty, True passes one entry per slot (pKF2, or the third keyframe for other_kf)."""

    def __init__(self, pb, extra: int = 3, seed: int = 0, null_match=(), null_kf1=(), bad1=(), bad2=(), unindexed1=(), unindexed2=(), other_kf=(),
                 matched_kf=None):
        from . import synth_sim3_ransac as ss
        rng = np.random.RandomState(seed)
        n = pb.n
        self.pb, self.n, self.n1 = pb, n, n + extra
        self.slot = np.sort(rng.permutation(self.n1)[:n]).astype(np.int32)
        self.key1, self.key2 = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
        self.level_sigma2 = ss.level_sigma2()
        self.camera_type = [int(pb.camera_type1), int(pb.camera_type2), int(pb.camera_type2)]
        self.camera = [np.asarray(pb.camera1, np.float32), np.asarray(pb.camera2, np.float32), np.asarray(pb.camera2, np.float32)]
        self.Rcw = [np.asarray(pb.Rcw1, np.float32), np.asarray(pb.Rcw2, np.float32), np.eye(3, dtype=np.float32)]
        self.tcw = [np.asarray(pb.tcw1, np.float32), np.asarray(pb.tcw2, np.float32), np.zeros(3, np.float32)]
        self.octave = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, 7, np.int32)]
        self.octave[0][self.key1], self.octave[1][self.key2] = pb.octave1, pb.octave2
        self.world = np.concatenate([pb.world1, pb.world2]).astype(np.float32)
        self.bad = np.zeros(2 * n, np.uint8)
        self.bad[list(bad1)] = 1
        self.bad[[n + i for i in bad2]] = 1
        self.index_in_kf = np.full((2 * n, 3), -1, np.int32)
        self.index_in_kf[:n, 0], self.index_in_kf[n:, 1] = self.key1, self.key2
        self.index_in_kf[list(unindexed1), 0] = -1
        for i in list(unindexed2) + list(other_kf):
            self.index_in_kf[n + i, 1] = -1
        for i in other_kf:
            self.index_in_kf[n + i, 2] = self.key2[i]
        self.kf1_mp = np.full(self.n1, -1, np.int32)
        self.kf1_mp[self.slot] = np.arange(n)
        self.kf1_mp[self.slot[list(null_kf1)]] = -1
        self.matched12 = np.full(self.n1, -1, np.int32)
        self.matched12[self.slot] = n + np.arange(n)
        self.matched12[self.slot[list(null_match)]] = -1
        self.matched_kf = None
        if matched_kf:
            self.matched_kf = np.ones(self.n1, np.int32)
            self.matched_kf[self.slot[list(other_kf)]] = 2
        self.fix_scale = int(pb.fix_scale)

    def c_struct(self):
        sc, keep = capi.HostSim3Scene(), []
        sc.n_kf = 3
        for k in range(3):
            sc.camera_type[k] = self.camera_type[k]
            sc.camera[k][:] = [float(v) for v in self.camera[k]]
            sc.Rcw[k][:] = [float(v) for v in self.Rcw[k].reshape(9)]
            sc.tcw[k][:] = [float(v) for v in self.tcw[k]]
            sc.n_keys[k] = self.n
            xy = np.zeros((self.n, 2), np.float32)
            keep += [xy, np.ascontiguousarray(self.octave[k], np.int32)]
            sc.xy[k], sc.octave[k] = capi.ptr(keep[-2], capi.c_float_p), capi.ptr(keep[-1], capi.c_int32_p)
        keep += [np.ascontiguousarray(a) for a in (self.level_sigma2, self.world, self.bad, self.index_in_kf, self.kf1_mp, self.matched12)]
        sc.n_levels, sc.level_sigma2 = len(self.level_sigma2), capi.ptr(keep[-6], capi.c_float_p)
        sc.n_points, sc.world, sc.bad = 2 * self.n, capi.ptr(keep[-5], capi.c_float_p), capi.ptr(keep[-4], capi.c_uint8_p)
        sc.index_in_kf = capi.ptr(keep[-3], capi.c_int32_p)
        sc.n1, sc.kf1_mp, sc.matched12 = self.n1, capi.ptr(keep[-2], capi.c_int32_p), capi.ptr(keep[-1], capi.c_int32_p)
        if self.matched_kf is not None:
            keep.append(np.ascontiguousarray(self.matched_kf, np.int32))
            sc.matched_kf = capi.ptr(keep[-1], capi.c_int32_p)
        sc.fix_scale = self.fix_scale
        return sc, keep


class Sim3Solver:
    """A Sim3Solver (include/Sim3Solver.h) of the stand-in classes built from a Sim3Scene."""

    STATE = ("N", "n1", "min_inliers", "max_iterations", "iterations", "best_inliers", "has_answer", "on_device")

    def __init__(self, scene: Sim3Scene, ransac=None):
        self.lib = capi.load_host_library()
        self.scene, self.n1 = scene, scene.n1
        sc, _keep = scene.c_struct()
        self.handle = self.lib.osh_host_sim3_solver_create(C.byref(sc))
        if not self.handle:
            raise RuntimeError("osh_host_sim3_solver_create refused the arguments")
        if ransac is not None:
            self.set_ransac(*ransac)

    def set_ransac(self, probability=0.99, min_inliers=6, max_iterations=300):
        if self.lib.osh_host_sim3_solver_set_ransac(self.handle, probability, min_inliers, max_iterations) != 0:
            raise RuntimeError("osh_host_sim3_solver_set_ransac")

    def state(self) -> dict:
        out = np.zeros(8, np.int32)
        self.lib.osh_host_sim3_solver_state(self.handle, capi.ptr(out, capi.c_int32_p))
        return dict(zip(self.STATE, (int(v) for v in out)))

    def pack(self) -> dict:
        n = self.state()["N"]
        f = lambda *shape: np.zeros(shape, np.float32)
        o = dict(x3dc1=f(n, 3), x3dc2=f(n, 3), p1im1=f(n, 2), p2im2=f(n, 2), max_error1=f(n), max_error2=f(n), indices1=np.zeros(n, np.int32))
        rc = self.lib.osh_host_sim3_solver_pack(self.handle, *[capi.ptr(o[k], capi.c_float_p) for k in list(o)[:6]], capi.ptr(o["indices1"], capi.c_int32_p))
        if rc != 0:
            raise RuntimeError(f"osh_host_sim3_solver_pack -> {rc}")
        return o

    def best(self) -> dict:
        n = self.state()["N"]
        o = dict(T12=np.zeros((4, 4), np.float32), R=np.zeros((3, 3), np.float32), t=np.zeros(3, np.float32), s=np.zeros(1, np.float32))
        flags = np.zeros(max(n, 1), np.uint8)
        rc = self.lib.osh_host_sim3_solver_best(self.handle, *[capi.ptr(v, capi.c_float_p) for v in o.values()], capi.ptr(flags, capi.c_uint8_p))
        if rc != 0:
            raise RuntimeError(f"osh_host_sim3_solver_best -> {rc}")
        o["flags"] = flags[:n].astype(bool)
        return o

    def iterate(self, n_iterations: int, mode: int = 1) -> dict:
        """mode 0: the four-argument iterate, 1: the one with bConverge, 3: find."""
        return sim3_iterate([self], n_iterations, mode)[0]

    def prepare(self, capacity: int = 1024):
        """The sets the device call of the next iterate would run: [count, 3] (an empty array when no call is due)."""
        sets = np.zeros((capacity, 3), np.int32)
        rc = self.lib.osh_host_sim3_solver_prepare(self.handle, capacity, capi.ptr(sets, capi.c_int32_p))
        if rc < 0:
            raise RuntimeError(f"osh_host_sim3_solver_prepare -> {rc}")
        return sets[:min(rc, capacity)]

    def keep(self, record, record_count, record_T, record_flags):
        """Hands the prepared round a given answer: the record iterations, their counts, transforms [k, 13] and flags [k, N]."""
        n = self.state()["N"]
        words = capi.ransac_mask_words(n)
        record, record_count = np.ascontiguousarray(record, np.int32), np.ascontiguousarray(record_count, np.int32)
        T = np.ascontiguousarray(record_T, np.float32).reshape(-1, 13)
        bits = np.zeros((len(record), words * 32), np.uint8)
        if len(record):
            bits[:, :n] = np.asarray(record_flags, bool).reshape(len(record), n)
        mask = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.uint32)
        rc = self.lib.osh_host_sim3_solver_keep(self.handle, len(record), capi.ptr(record, capi.c_int32_p), capi.ptr(record_count, capi.c_int32_p),
                                                capi.ptr(T, capi.c_float_p), capi.ptr(mask, capi.c_uint32_p))
        if rc != 0:
            raise RuntimeError(f"osh_host_sim3_solver_keep -> {rc}")

    def replay(self, n_iterations: int, five: bool = True) -> dict:
        no_more, conv, n_in = np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.int32)
        inl, T = np.zeros(max(self.n1, 1), np.uint8), np.zeros(16, np.float32)
        rc = self.lib.osh_host_sim3_solver_replay(self.handle, int(n_iterations), int(five), self.n1, capi.ptr(no_more, capi.c_uint8_p),
                                                  capi.ptr(n_in, capi.c_int32_p), capi.ptr(conv, capi.c_uint8_p), capi.ptr(inl, capi.c_uint8_p),
                                                  capi.ptr(T, capi.c_float_p))
        if rc != 0:
            raise RuntimeError(f"osh_host_sim3_solver_replay -> {rc}")
        return dict(no_more=bool(no_more[0]), converged=bool(conv[0]), n_inliers=int(n_in[0]), inliers=inl[:self.n1].astype(bool), T12=T.reshape(4, 4))

    def close(self):
        if self.handle:
            self.lib.osh_host_sim3_solver_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sim3_iterate(solvers, n_iterations: int, mode: int = 2) -> list:
    """Every Sim3Solver once: mode 0 / 1 the two iterate overloads one by one, 2 Sim3Solver::IterateBatch (one device call), 3 find.
    Per solver a dict with no_more, converged, n_inliers, inliers [n1] and T12 [4, 4]."""
    lib = capi.load_host_library()
    S = len(solvers)
    m = max([s.n1 for s in solvers], default=0)
    handles = (C.c_void_p * max(S, 1))(*[s.handle for s in solvers])
    no_more, conv, n_in = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros(S, np.int32)
    inl, T = np.zeros((S, max(m, 1)), np.uint8), np.zeros((S, 16), np.float32)
    rc = lib.osh_host_sim3_solver_iterate(S, handles, int(n_iterations), int(mode), m, capi.ptr(no_more, capi.c_uint8_p), capi.ptr(n_in, capi.c_int32_p),
                                          capi.ptr(conv, capi.c_uint8_p), capi.ptr(inl, capi.c_uint8_p), capi.ptr(T, capi.c_float_p))
    if rc != 0:
        raise RuntimeError(f"osh_host_sim3_solver_iterate -> {rc}")
    return [dict(no_more=bool(no_more[k]), converged=bool(conv[k]), n_inliers=int(n_in[k]), inliers=inl[k, :s.n1].astype(bool),
                 T12=T[k].reshape(4, 4).copy()) for k, s in enumerate(solvers)]


def create_new_map_points(scene, coarse: bool = True, new_keyframe_waiting: bool = False, capacity: int = 4096) -> dict:
    """LocalMapping::CreateNewMapPoints on the stand-in classes built from a synth_newpoints.Scene (osh_host_create_new_map_points).
    Keyframe 0 is the current one, keyframe 1 + k neighbour k; the first two neighbours are covisibles, the third is reached
    through mPrevKF (an inertial scene) or is a covisible too.  Every matched feature pair shares a descriptor and a vocabulary node
    of its own.  Returns the created points in creation order (neighbour as a segment index, idx1, idx2, x3d, n_obs, flags) and
    poses [n_kf, 2, 24]: Rcw tcw Rwc Ow of every keyframe's left and right pose as handed to the device."""
    from . import synth_fisheye as sf
    from . import synth_newpoints as sn
    lib = capi.load_host_library()
    segs = scene.segments
    k1 = segs[0].kf1
    N = k1.n_keys
    rng = np.random.default_rng(12345)
    desc1 = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    keep = []

    def keyframe(c, kf, idx, pt, octave, ur, depth, node_of, desc, has_mp, mp_pos, prev):
        n = kf.n_keys
        a = dict(xy=np.zeros((n, 2), np.float32), octave=np.zeros(n, np.int32), ur=np.full(n, -1, np.float32), depth=np.full(n, -1, np.float32),
                 desc=np.ascontiguousarray(desc), has_mp=np.ascontiguousarray(has_mp, np.uint8), mp_pos=np.ascontiguousarray(mp_pos, np.float32))
        a["xy"][idx], a["octave"][idx], a["ur"][idx], a["depth"][idx] = pt, octave, ur, depth
        nodes = sorted(set(int(v) for v in node_of.values()))
        feats = {v: [] for v in nodes}
        for f in sorted(node_of):
            feats[int(node_of[f])].append(f)
        a["node_id"] = np.asarray(nodes, np.int32)
        a["node_off"] = np.concatenate([[0], np.cumsum([len(feats[v]) for v in nodes])]).astype(np.int32)
        a["node_feat"] = np.asarray([f for v in nodes for f in feats[v]], np.int32)
        keep.append(a)
        c.n, c.n_left = n, int(kf.n_left)
        for field, key, typ in (("xy", "xy", capi.c_float_p), ("octave", "octave", capi.c_int32_p), ("desc", "desc", capi.c_uint8_p),
                                ("u_right", "ur", capi.c_float_p), ("depth", "depth", capi.c_float_p), ("has_mp", "has_mp", capi.c_uint8_p),
                                ("mp_pos", "mp_pos", capi.c_float_p), ("node_id", "node_id", capi.c_int32_p),
                                ("node_off", "node_off", capi.c_int32_p), ("node_feat", "node_feat", capi.c_int32_p)):
            setattr(c, field, capi.ptr(a[key], typ))
        c.n_nodes = len(nodes)
        R = kf.pose.Rcw.astype(np.float64)
        c.pose_qt[:] = [float(np.float32(v)) for v in np.concatenate([synth._quat_from_R(R), kf.pose.tcw.astype(np.float64)])]
        c.trl_qt[:] = [float(np.float32(v)) for v in np.concatenate([synth._quat_from_R(sf.rotation(sn.RIG_ROTVEC)), np.asarray(sn.RIG_T)])]
        c.camera_kb8 = int(kf.camera.type == sn.KB8)
        c.camera[:] = [float(v) for v in kf.camera.params]
        c.has_camera2 = int(kf.camera2 is not None)
        if kf.camera2 is not None:
            c.camera2[:] = [float(v) for v in kf.camera2.params]
        c.mbf, c.mb, c.n_levels, c.scale_factor, c.prev = float(kf.mbf), float(kf.mb), len(kf.scale_factors), float(np.float32(sf.SCALE)), prev

    n_kf = 1 + len(segs)
    ckf = (capi.HostNewPointKf * n_kf)()
    # the current keyframe: its features over all segments (a shared feature carries the same keypoint in each)
    idx1 = np.concatenate([s.idx1 for s in segs])
    cat = lambda f: np.concatenate([getattr(s, f) for s in segs])
    inertial_walk = bool(scene.inertial) and len(segs) == 3
    keyframe(ckf[0], k1, idx1, cat("pt1"), cat("octave1"), cat("u_right1"), cat("depth1"), {int(i): int(i) for i in idx1}, desc1,
             np.zeros(N, np.uint8), np.zeros((N, 3), np.float32), 3 if inertial_walk else -1)
    for k, s in enumerate(segs):
        d = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        d[s.idx2] = desc1[s.idx1]
        has = np.zeros(N, np.uint8)
        pos = np.zeros((N, 3), np.float32)
        feats, p = scene.map_points[k]
        has[feats], pos[feats] = 1, p
        keyframe(ckf[1 + k], s.kf2, s.idx2, s.pt2, s.octave2, s.u_right2, s.depth2, {int(b): int(a) for a, b in zip(s.idx1, s.idx2)}, d, has, pos,
                 1 if (inertial_walk and k == 2) else -1)
    sc = capi.HostNewPointScene()
    nb = np.asarray([1, 2] if inertial_walk else list(range(1, n_kf)), np.int32)
    sc.n_kf, sc.kf, sc.n_neighbours, sc.neighbours = n_kf, ckf, len(nb), capi.ptr(nb, capi.c_int32_p)
    sc.monocular, sc.inertial, sc.far_points, sc.th_far_points = int(scene.monocular), int(scene.inertial), int(scene.far_points), float(scene.th_far_points)
    sc.recently_lost = sc.inertial_ba2 = int(coarse)
    sc.new_keyframe_waiting = int(new_keyframe_waiting)
    o = dict(neighbour=np.zeros(capacity, np.int32), idx1=np.zeros(capacity, np.int32), idx2=np.zeros(capacity, np.int32),
             x3d=np.zeros((capacity, 3), np.float32), n_obs=np.zeros(capacity, np.int32), flags=np.zeros(capacity, np.int32))
    poses = np.zeros((n_kf, 2, 24), np.float32)
    n = lib.osh_host_create_new_map_points(C.byref(sc), capacity, capi.ptr(o["neighbour"], capi.c_int32_p), capi.ptr(o["idx1"], capi.c_int32_p),
                                           capi.ptr(o["idx2"], capi.c_int32_p), capi.ptr(o["x3d"], capi.c_float_p),
                                           capi.ptr(o["n_obs"], capi.c_int32_p), capi.ptr(o["flags"], capi.c_int32_p), capi.ptr(poses, capi.c_float_p))
    if n < 0 or n > capacity:
        raise RuntimeError(f"osh_host_create_new_map_points returned {n}")
    out = {k: v[:n] for k, v in o.items()}
    out["neighbour"] = out["neighbour"] - 1          # keyframe index -> segment index
    out["poses"] = poses
    return out


def orb_fast_cpu(frames):
    """csrc/orb_fast.h on the host in one thread (osh_host_orb_fast_cpu): the per-frame dicts of OrbMatcher.fast_detect, ms."""
    from . import orb
    return orb.fast_cpu(frames)


def orb_ic_angle_cpu(items):
    """IC_Angle of csrc/orb_fast.h on the host in one thread (osh_host_orb_ic_angle_cpu): per-item dicts angle / m10 / m01, ms."""
    from . import orb
    return orb.ic_angle_cpu(items)


def orbextractor_compute_keypoints(pyramid, nfeatures=1000, scale_factor=1.2, ini_th=20, min_th=7, nlevels=None, border=0) -> dict:
    """ORBextractor::ComputeKeyPointsOctTree of the stand-in class on a pyramid (a list of uint8 levels) through
    osh_host_orbextractor_compute_keypoints.  nlevels: of the extractor (default: the pyramid's; more than the pyramid has shows the
    refusal).  Returns level_count and the keypoints level after level (xy, response, angle, size, octave), the candidates every
    DistributeOctTree call received (cand_level_count, cand_xy, cand_response, cand_args [nlevels, 6]: minX maxX minY maxY nFeatures
    level), and the extractor's features_per_level and scale_factors."""
    from . import orb
    lib = capi.load_host_library()
    nlevels = len(pyramid) if nlevels is None else int(nlevels)
    rows = np.asarray([p.shape[0] for p in pyramid], np.int32)
    cols = np.asarray([p.shape[1] for p in pyramid], np.int32)
    pixels = np.concatenate([np.ascontiguousarray(p, np.uint8).ravel() for p in pyramid]) if len(pyramid) else np.zeros(1, np.uint8)
    cin = capi.HostOrbExtractorInput()
    cin.nfeatures, cin.scale_factor, cin.nlevels, cin.ini_th, cin.min_th = int(nfeatures), float(scale_factor), nlevels, int(ini_th), int(min_th)
    cin.n_images, cin.border = len(pyramid), int(border)
    cin.rows, cin.cols, cin.pixels = capi.ptr(rows, capi.c_int32_p), capi.ptr(cols, capi.c_int32_p), capi.ptr(pixels, capi.c_uint8_p)
    arrays = lambda cap, cand_cap: dict(
        level_count=np.zeros(max(nlevels, 1), np.int32), xy=np.zeros((cap, 2), np.float32), response=np.zeros(cap, np.float32),
        angle=np.zeros(cap, np.float32), size=np.zeros(cap, np.float32), octave=np.zeros(cap, np.int32),
        cand_level_count=np.zeros(max(nlevels, 1), np.int32), cand_xy=np.zeros((cand_cap, 2), np.float32),
        cand_response=np.zeros(cand_cap, np.float32), cand_args=np.zeros((max(nlevels, 1), 6), np.int32),
        features_per_level=np.zeros(max(nlevels, 1), np.int32), scale_factors=np.zeros(max(nlevels, 1), np.float32))
    _n, o = orb.counted_call(lib.osh_host_orbextractor_compute_keypoints, "osh_host_orbextractor_compute_keypoints", cin, capi.HostOrbExtractorOutput,
                             "cand_capacity", arrays, lambda n, o: (n, int(o["cand_level_count"].sum())))
    return {k: v[:nlevels] if k in ("level_count", "cand_level_count", "cand_args", "features_per_level", "scale_factors") else v for k, v in o.items()}


def orbextractor_distribute_device(xy, response, width, height, n_features) -> dict:
    """ORBextractor::DistributeOctTreeDevice of a stand-in extractor on one list of candidates (relative to minBorder) through
    osh_host_orbextractor_distribute_device: a dict with index (the kept input indices in result order), xy, response of the kept
    keypoints and distribute_calls, the number of DistributeOctTree calls the member made."""
    lib = capi.load_host_library()
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    response = np.ascontiguousarray(response, np.float32).reshape(-1)
    n = len(response)
    lst = capi.OctreeList(n, capi.ptr(xy, capi.c_float_p), capi.ptr(response, capi.c_float_p), int(width), int(height), int(n_features))
    index, kxy, kresp = np.full(max(n, 1), -1, np.int32), np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.float32)
    calls = C.c_int32(-1)
    kept = lib.osh_host_orbextractor_distribute_device(C.byref(lst), n, capi.ptr(index, capi.c_int32_p), capi.ptr(kxy, capi.c_float_p),
                                                       capi.ptr(kresp, capi.c_float_p), C.byref(calls))
    if kept < 0:
        raise RuntimeError(f"osh_host_orbextractor_distribute_device returned {kept}")
    return dict(index=index[:kept], xy=kxy[:kept], response=kresp[:kept], distribute_calls=int(calls.value))


def orbextractor_extract_batch(images, lappings, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, keep_pyramid=True) -> list:
    """ORBextractor::ExtractBatch of one stand-in extractor per image (None or an empty array: an empty image) with its lapping
    area, through osh_host_orbextractor_extract_batch: per image a dict with ret (monoIndex), desc_rows, token (mnPyramidToken),
    pyramid (mvImagePyramid after the call, a list of levels), xy, angle, size, response, octave, descriptors [n, 32] of
    _keypoints, and call_ms, the wall time of the one ExtractBatch call."""
    from . import orb
    lib = capi.load_host_library()
    n = len(images)
    cin = (capi.HostExtractInput * max(n, 1))()
    imgs = [orb.fill_host_extract_input(cin[i], im, nfeatures, scale_factor, nlevels, ini_th, min_th, lappings[i]) for i, im in enumerate(images)]
    cap = [2 * int(nfeatures) + 300 * int(nlevels)] * n
    pix = [int(sum((img.shape[0] + 2) * (img.shape[1] + 2) for _ in range(nlevels))) if img.size else 1 for img in imgs]
    outs, cout = [], (capi.HostExtractOutput * max(n, 1))()
    for i in range(n):
        o = dict(level_rows=np.zeros(nlevels, np.int32), level_cols=np.zeros(nlevels, np.int32), pyramid=np.zeros(pix[i], np.uint8),
                 xy=np.zeros((cap[i], 2), np.float32), angle=np.zeros(cap[i], np.float32), size=np.zeros(cap[i], np.float32),
                 response=np.zeros(cap[i], np.float32), octave=np.zeros(cap[i], np.int32), descriptors=np.zeros((cap[i], 32), np.uint8),
                 ret=np.zeros(1, np.int32), desc_rows=np.zeros(1, np.int32), pixels_needed=np.zeros(1, np.int32), call_ms=np.zeros(1, np.float64))
        cout[i].capacity, cout[i].pixel_capacity = cap[i], pix[i]
        orb._wire_outputs(cout[i], o)
        outs.append(o)
    tokens = (C.c_uint64 * max(n, 1))()
    rc = lib.osh_host_orbextractor_extract_batch(n, cin, cout, int(bool(keep_pyramid)), tokens)
    if rc != 0:
        raise RuntimeError(f"osh_host_orbextractor_extract_batch returned {rc}")
    res = []
    for i, o in enumerate(outs):
        k = int(o["desc_rows"][0])
        d = dict(ret=int(o["ret"][0]), desc_rows=k, token=int(tokens[i]), call_ms=float(o["call_ms"][0]))
        for name in ("xy", "angle", "size", "response", "octave", "descriptors"):
            d[name] = o[name][:k]
        d["pyramid"] = orb.cut_levels(o["pyramid"], zip(o["level_rows"].tolist(), o["level_cols"].tolist()))
        res.append(d)
    return res


def _fill_host_raw_image(r, it, keep: list) -> tuple:
    """A capi.HostRawImage from an item dict(image, optionally order, map_x / map_y, out_shape); the arrays its pointers refer to are
    added to `keep`.  Returns the (rows, cols) of the prepared image."""
    img = None if it.get("image") is None else np.ascontiguousarray(it["image"], np.uint8)
    r.rgb = int(it.get("order", "rgb") == "rgb")
    shape = (0, 0)
    if img is not None and img.size:
        r.rows, r.cols, r.channels = img.shape[0], img.shape[1], 1 if img.ndim == 2 else img.shape[2]
        r.pixels = capi.ptr(img, capi.c_uint8_p)
        shape = img.shape[:2]
    else:
        r.channels = 1
    if it.get("map_x") is not None:
        mx, my = np.ascontiguousarray(it["map_x"], np.float32), np.ascontiguousarray(it["map_y"], np.float32)
        r.map_rows, r.map_cols = mx.shape
        r.map_x, r.map_y = capi.ptr(mx, capi.c_float_p), capi.ptr(my, capi.c_float_p)
        keep.append((mx, my))
        shape = mx.shape
    if it.get("out_shape") is not None:
        r.new_rows, r.new_cols = int(it["out_shape"][0]), int(it["out_shape"][1])
        shape = (max(r.new_rows, 0), max(r.new_cols, 0))
    keep.append(img)
    return tuple(shape)


def orbextractor_extract_batch_raw(items, lappings, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, keep_pyramid=True,
                                   want_gray=True) -> list:
    """ORBextractor::ExtractBatchRaw of one stand-in extractor per item dict(image uint8 [rows, cols] or [rows, cols, 3 | 4] (None: an
    empty image), optionally order ("rgb" / "bgr"), map_x / map_y (float32 [rows, cols]: a RectifyMap of its own), out_shape), through
    osh_host_orbextractor_extract_batch_raw: per item the dict of orbextractor_extract_batch and, with want_gray, gray (the image of
    *pvGray; None when it came back empty)."""
    from . import orb
    lib = capi.load_host_library()
    n = len(items)
    cin = (capi.HostExtractInput * max(n, 1))()
    raw = (capi.HostRawImage * max(n, 1))()
    keep, shapes = [], []
    for i, it in enumerate(items):
        orb.fill_host_extract_input(cin[i], None, nfeatures, scale_factor, nlevels, ini_th, min_th, lappings[i])
        shapes.append(_fill_host_raw_image(raw[i], it, keep))
    cap = [2 * int(nfeatures) + 300 * int(nlevels)] * n
    pix = [int((s[0] + 2) * (s[1] + 2) * nlevels) if s[0] * s[1] else 1 for s in shapes]
    outs, cout = [], (capi.HostExtractOutput * max(n, 1))()
    for i in range(n):
        o = dict(level_rows=np.zeros(nlevels, np.int32), level_cols=np.zeros(nlevels, np.int32), pyramid=np.zeros(pix[i], np.uint8),
                 xy=np.zeros((cap[i], 2), np.float32), angle=np.zeros(cap[i], np.float32), size=np.zeros(cap[i], np.float32),
                 response=np.zeros(cap[i], np.float32), octave=np.zeros(cap[i], np.int32), descriptors=np.zeros((cap[i], 32), np.uint8),
                 ret=np.zeros(1, np.int32), desc_rows=np.zeros(1, np.int32), pixels_needed=np.zeros(1, np.int32), call_ms=np.zeros(1, np.float64))
        cout[i].capacity, cout[i].pixel_capacity = cap[i], pix[i]
        orb._wire_outputs(cout[i], o)
        outs.append(o)
    tokens = (C.c_uint64 * max(n, 1))()
    grays = [np.full(max(s[0] * s[1], 1), 167, np.uint8) for s in shapes]
    gptr = (capi.c_uint8_p * max(n, 1))(*[capi.ptr(g, capi.c_uint8_p) for g in grays])
    gcap = np.asarray([g.size for g in grays] or [0], np.int32)
    grows, gcols = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)
    rc = lib.osh_host_orbextractor_extract_batch_raw(n, cin, raw, cout, int(bool(keep_pyramid)), tokens, gptr if want_gray else None,
                                                     capi.ptr(gcap, capi.c_int32_p), capi.ptr(grows, capi.c_int32_p), capi.ptr(gcols, capi.c_int32_p))
    if rc != 0:
        raise RuntimeError(f"osh_host_orbextractor_extract_batch_raw returned {rc}")
    res = []
    for i, o in enumerate(outs):
        k = int(o["desc_rows"][0])
        d = dict(ret=int(o["ret"][0]), desc_rows=k, token=int(tokens[i]), call_ms=float(o["call_ms"][0]))
        for name in ("xy", "angle", "size", "response", "octave", "descriptors"):
            d[name] = o[name][:k]
        d["pyramid"] = orb.cut_levels(o["pyramid"], zip(o["level_rows"].tolist(), o["level_cols"].tolist()))
        if want_gray:
            gr, gc = int(grows[i]), int(gcols[i])
            d["gray"] = grays[i][:gr * gc].reshape(gr, gc) if gr > 0 and gr * gc <= grays[i].size else None
        res.append(d)
    return res


def frame_extract_and_match_stereo(left, right, bf, b, raw=False, chain=False, want_gray=False, nfeatures=1000, scale_factor=1.2, nlevels=8,
                                   ini_th=20, min_th=7) -> dict:
    """Frame::ExtractAndMatchStereo of a stand-in Frame with two stand-in extractors through osh_host_frame_extract_and_match_stereo.
    left / right: uint8 images (None: an empty image), or with `raw` the items of orbextractor_extract_batch_raw.  chain: the two
    calls the member replaces instead, ExtractBatch(Raw) with bKeepPyramid and ComputeStereoMatches.  A dict with left / right (the
    dicts of orbextractor_extract_batch for mvKeys / mDescriptors and mvKeysRight / mDescriptorsRight), N, u_right, depth (mvuRight
    and mvDepth), n_right and call_ms, the wall time of the member calls alone; with want_gray the sides also carry gray."""
    from . import orb
    lib = capi.load_host_library()
    cin = (capi.HostExtractInput * 2)()
    rawc = (capi.HostRawImage * 2)()
    keep, shapes = [], []
    for i, side in enumerate((left, right)):
        if raw:
            orb.fill_host_extract_input(cin[i], None, nfeatures, scale_factor, nlevels, ini_th, min_th)
            shapes.append(_fill_host_raw_image(rawc[i], side, keep))
        else:
            img = orb.fill_host_extract_input(cin[i], side, nfeatures, scale_factor, nlevels, ini_th, min_th)
            keep.append(img)
            shapes.append(img.shape if img.size else (0, 0))
    cap = 2 * int(nfeatures) + 300 * int(nlevels)
    outs, cout = [], (capi.HostExtractOutput * 2)()
    for i in range(2):
        pix = int((shapes[i][0] + 2) * (shapes[i][1] + 2) * nlevels) if shapes[i][0] * shapes[i][1] else 1
        o = dict(level_rows=np.zeros(nlevels, np.int32), level_cols=np.zeros(nlevels, np.int32), pyramid=np.zeros(pix, np.uint8),
                 xy=np.zeros((cap, 2), np.float32), angle=np.zeros(cap, np.float32), size=np.zeros(cap, np.float32),
                 response=np.zeros(cap, np.float32), octave=np.zeros(cap, np.int32), descriptors=np.zeros((cap, 32), np.uint8),
                 ret=np.zeros(1, np.int32), desc_rows=np.zeros(1, np.int32), pixels_needed=np.zeros(1, np.int32))
        cout[i].capacity, cout[i].pixel_capacity = cap, pix
        orb._wire_outputs(cout[i], o)
        outs.append(o)
    tokens = (C.c_uint64 * 2)()
    u_right, depth = np.full(cap, 5, np.float32), np.full(cap, 5, np.float32)
    counts = np.full(4, -1, np.int32)
    grays = [np.full(max(s[0] * s[1], 1), 167, np.uint8) for s in shapes]
    gptr = (capi.c_uint8_p * 2)(*[capi.ptr(g, capi.c_uint8_p) for g in grays])
    gcap = np.asarray([g.size for g in grays], np.int32)
    grows, gcols = np.full(2, -1, np.int32), np.full(2, -1, np.int32)
    ms = C.c_double(0)
    rc = lib.osh_host_frame_extract_and_match_stereo(cin, rawc if raw else None, float(bf), float(b), int(bool(chain)), cout, tokens, cap,
                                                     capi.ptr(u_right, capi.c_float_p), capi.ptr(depth, capi.c_float_p), capi.ptr(counts, capi.c_int32_p),
                                                     gptr if want_gray else None, capi.ptr(gcap, capi.c_int32_p), capi.ptr(grows, capi.c_int32_p),
                                                     capi.ptr(gcols, capi.c_int32_p), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_frame_extract_and_match_stereo returned {rc}")
    sides = []
    for i, o in enumerate(outs):
        k = int(o["desc_rows"][0])
        d = dict(desc_rows=k, token=int(tokens[i]))
        for name in ("xy", "angle", "size", "response", "octave", "descriptors"):
            d[name] = o[name][:k]
        d["pyramid"] = orb.cut_levels(o["pyramid"], zip(o["level_rows"].tolist(), o["level_cols"].tolist()))
        if want_gray:
            gr, gc = int(grows[i]), int(gcols[i])
            d["gray"] = grays[i][:gr * gc].reshape(gr, gc) if gr > 0 and gr * gc <= grays[i].size else None
        sides.append(d)
    return dict(left=sides[0], right=sides[1], N=int(counts[0]), u_right=u_right[:max(int(counts[1]), 0)], depth=depth[:max(int(counts[2]), 0)],
                n_right=int(counts[3]), call_ms=float(ms.value))
