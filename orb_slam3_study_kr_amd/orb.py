"""Python driver over the ORB matching C-ABI (include/orbslam3_hip.h, osh_orb_*)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi
from .synth import OrbPair


class OrbMatcher:
    def __init__(self, device: int = 0):
        self.lib = capi.load_library()
        self.ctx = C.c_void_p()
        capi.check(self.lib.osh_orb_create(device, C.byref(self.ctx)), "osh_orb_create", self.lib)
        self._shape = None
        self._keep = None
        self.device = device

    def close(self):
        if self.ctx:
            self.lib.osh_orb_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upload(self, pairs: list[OrbPair], windowed: bool = False):
        n_pairs = len(pairs)
        nq, nt = pairs[0].query_desc.shape[0], pairs[0].train_desc.shape[0]
        q = np.ascontiguousarray(np.stack([p.query_desc for p in pairs]), dtype=np.uint8)
        t = np.ascontiguousarray(np.stack([p.train_desc for p in pairs]), dtype=np.uint8)
        lev = np.ascontiguousarray(np.stack([p.train_level for p in pairs]), dtype=np.int32)
        b = capi.OrbBatch()
        b.n_pairs, b.n_query, b.n_train = n_pairs, nq, nt
        b.query_desc, b.train_desc = capi.ptr(q, capi.c_uint8_p), capi.ptr(t, capi.c_uint8_p)
        b.train_level = capi.ptr(lev, capi.c_int32_p)
        keep = [q, t, lev]
        if windowed:
            off = np.ascontiguousarray(np.stack([p.cand_off for p in pairs]), dtype=np.int32)
            idx = np.ascontiguousarray(np.concatenate([p.cand_idx for p in pairs]), dtype=np.int32)
            lens = np.array([p.cand_idx.shape[0] for p in pairs], dtype=np.int64)
            base = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)[:-1]]), dtype=np.int64)
            if idx.size == 0:
                idx = np.zeros(1, dtype=np.int32)
            b.cand_off, b.cand_idx = capi.ptr(off, capi.c_int32_p), capi.ptr(idx, capi.c_int32_p)
            b.pair_cand_base = capi.ptr(base, capi.c_int64_p)
            keep += [off, idx, base]
            self._list_total = int(lens.sum())
        self._keep = keep
        self._shape = (n_pairs, nq)
        self._n_train = nt
        capi.check(self.lib.osh_orb_upload(self.ctx, C.byref(b)), "osh_orb_upload", self.lib)

    def upload_grid(self, query_desc, train_desc, train_level, train_xy, query_window, query_levels, train_uright=None,
                    train_skip=None, query_uright=None):
        """One frame pair whose candidates are generated on the device from the train frame's grid
        (Frame::GetFeaturesInArea, src/Frame.cc:658-722): query_window [nq,3] = x, y, r; query_levels [nq,2] = min, max."""
        from . import synth
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        q = np.ascontiguousarray(query_desc, dtype=np.uint8)
        t = np.ascontiguousarray(train_desc, dtype=np.uint8)
        lev = np.ascontiguousarray(train_level, dtype=np.int32)
        b = capi.OrbBatch()
        b.n_pairs, b.n_query, b.n_train = 1, q.shape[0], t.shape[0]
        b.query_desc, b.train_desc, b.train_level = capi.ptr(q, capi.c_uint8_p), capi.ptr(t, capi.c_uint8_p), capi.ptr(lev, capi.c_int32_p)
        g = capi.OrbGrid()
        keep = [q, t, lev, f32(train_xy), f32(query_window), np.ascontiguousarray(query_levels, dtype=np.int32)]
        g.train_xy, g.query_window, g.query_levels = capi.ptr(keep[3], capi.c_float_p), capi.ptr(keep[4], capi.c_float_p), capi.ptr(keep[5], capi.c_int32_p)
        if train_uright is not None:
            keep.append(f32(train_uright)); g.train_uright = capi.ptr(keep[-1], capi.c_float_p)
        if train_skip is not None:
            keep.append(np.ascontiguousarray(train_skip, dtype=np.uint8)); g.train_skip = capi.ptr(keep[-1], capi.c_uint8_p)
        if query_uright is not None:
            keep.append(f32(query_uright)); g.query_uright = capi.ptr(keep[-1], capi.c_float_p)
        g.min_x, g.min_y = 0.0, 0.0
        g.cell_w_inv = np.float32(synth.FRAME_GRID_COLS) / np.float32(synth.IMG_W)
        g.cell_h_inv = np.float32(synth.FRAME_GRID_ROWS) / np.float32(synth.IMG_H)
        g.cols, g.rows = synth.FRAME_GRID_COLS, synth.FRAME_GRID_ROWS
        self._keep = keep
        self._shape = (1, q.shape[0])
        self._n_train = t.shape[0]
        capi.check(self.lib.osh_orb_upload_grid(self.ctx, C.byref(b), C.byref(g)), "osh_orb_upload_grid", self.lib)

    def frustum(self, frame: "capi.FrustumFrame", pos, normal, min_dist, max_dist) -> dict:
        """Frame::isInFrustum (src/Frame.cc:513-587) for every map point of `pos` [n,3]; see osh_orb_frustum."""
        args, res, outs = frustum_args(pos, normal, min_dist, max_dist)
        capi.check(self.lib.osh_orb_frustum(self.ctx, C.byref(frame), C.byref(args[0]), C.byref(res)), "osh_orb_frustum", self.lib)
        return outs

    def list_distances(self):
        """osh_orb_list_distances: the Hamming distance of every (query, candidate) entry of the uploaded lists, pairs concatenated."""
        out = np.zeros(max(self._list_total, 1), dtype=np.int32)
        capi.check(self.lib.osh_orb_list_distances(self.ctx, capi.ptr(out, capi.c_int32_p)), "osh_orb_list_distances", self.lib)
        return out[:self._list_total]

    def match(self):
        capi.check(self.lib.osh_orb_match(self.ctx), "osh_orb_match", self.lib)

    def match_local_points(self, nn_ratio: float = 0.8, th_high: int = 100, occupied=None, query_blocks=None, n_train: int | None = None):
        """SearchByProjection(Frame&, vector<MapPoint*>&) with the sequential slot occupancy resolved on the device
        (osh_orb_match_local_points): (n_matches[n_pairs], assignment[n_pairs, n_train], query_slot[n_pairs, n_query], rounds)."""
        n_pairs, n_query = self._shape
        n_train = int(n_train if n_train is not None else self._n_train)
        occ = None if occupied is None else np.ascontiguousarray(occupied, dtype=np.uint8).reshape(n_pairs, n_train)
        blk = None if query_blocks is None else np.ascontiguousarray(query_blocks, dtype=np.uint8).reshape(n_pairs, n_query)
        assign = np.zeros((n_pairs, n_train), dtype=np.int32)
        n = np.zeros(n_pairs, dtype=np.int32)
        slot = np.zeros((n_pairs, n_query), dtype=np.int32)
        rounds = C.c_int32(0)
        capi.check(self.lib.osh_orb_match_local_points(self.ctx, float(nn_ratio), int(th_high), capi.ptr(occ, capi.c_uint8_p),
                                                       capi.ptr(blk, capi.c_uint8_p), capi.ptr(assign, capi.c_int32_p),
                                                       capi.ptr(n, capi.c_int32_p), capi.ptr(slot, capi.c_int32_p), C.byref(rounds)),
                   "osh_orb_match_local_points", self.lib)
        return n, assign, slot, int(rounds.value)

    def download(self) -> dict:
        names = ["best_idx", "best_dist", "second_dist", "best_level", "second_level", "second_idx"]
        outs = [np.zeros(self._shape, dtype=np.int32) for _ in names]
        capi.check(self.lib.osh_orb_download(self.ctx, *[capi.ptr(o, capi.c_int32_p) for o in outs]), "osh_orb_download", self.lib)
        return dict(zip(names, outs))

    def search(self, pairs: list[OrbPair], windowed: bool = False) -> dict:
        self.upload(pairs, windowed)
        self.match()
        return self.download()

    def distance_matrix(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.uint8)
        b = np.ascontiguousarray(b, dtype=np.uint8)
        out = np.zeros((a.shape[0], b.shape[0]), dtype=np.int32)
        capi.check(self.lib.osh_orb_distance_matrix(self.ctx, a.shape[0], b.shape[0], capi.ptr(a, capi.c_uint8_p),
                                                    capi.ptr(b, capi.c_uint8_p), capi.ptr(out, capi.c_int32_p)),
                   "osh_orb_distance_matrix", self.lib)
        return out

    def stereo_match(self, frames, stages: bool = False, borders=None) -> list:
        """Frame::ComputeStereoMatches (src/Frame.cc:816-986) for a batch of synth_stereo.StereoFrame in one osh_orb_stereo_match
        call: per frame a dict with u_right / depth, and with `stages` also best_right, hamming, sad [n, 11], best_inc, stage.
        borders: per frame the pixels of border around every pyramid level (None: contiguous levels); the levels are then handed
        over as views into larger images, row stride cols + 2 * border."""
        cf, cr, _keep, outs = stereo_args(frames, stages, borders)
        capi.check(self.lib.osh_orb_stereo_match(self.ctx, len(frames), cf, cr), "osh_orb_stereo_match", self.lib)
        return outs

    def stereo_match_resident(self, frames, tokens, stages: bool = False) -> list:
        """stereo_match on pyramids that are resident on this matcher's context, in one osh_orb_stereo_match_resident call: frames
        bring keypoints, scale factors, bf and b (their pyramids are not read), tokens[k] = (left_token, right_token) from
        pyramid_build, extract or extract_raw.  The per-frame dicts are stereo_match's."""
        cf, cr, _keep, outs = stereo_resident_args(frames, tokens, stages)
        capi.check(self.lib.osh_orb_stereo_match_resident(self.ctx, len(frames), cf, cr), "osh_orb_stereo_match_resident", self.lib)
        return outs

    def set_stereo_row_search(self, enable: bool):
        """The descriptor search of stereo_match_resident and extract_stereo: the row lists (default) or k_stereo_hamming."""
        capi.check(self.lib.osh_orb_stereo_set_row_search(self.ctx, int(bool(enable))), "osh_orb_stereo_set_row_search", self.lib)

    def extract_stereo(self, pairs, capacities=None, download: bool = False, stages: bool = False, raw: bool = False) -> list:
        """A rectified stereo frame per pair in ONE osh_orb_extract_stereo call: pairs are dict(left, right, bf, b), left / right
        items of extract() (of extract_raw() with `raw`).  Per pair a dict with left / right (the dicts of extract()) and stereo (the
        dict of stereo_match for the left keypoints in extract order, level-0 scaled on the device; None when a frame's arrays
        were too small).  capacities: the room of the 2 n frames, left then right; None: a first call with no room sizes them."""
        if capacities is None:
            sized = self.extract_stereo(pairs, [0] * (2 * len(pairs)), raw=raw)
            capacities = [r[side]["n_out"] for r in sized for side in ("left", "right")]
        pf, cf, cp, cr, cs, _keep, outs, souts = extract_stereo_args(pairs, capacities, download, stages, raw)
        capi.check(self.lib.osh_orb_extract_stereo(self.ctx, len(pairs), pf, cf, cp, cr, cs), "osh_orb_extract_stereo", self.lib)
        return _extract_stereo_outputs(cr, outs, souts)

    def extract_stereo_times(self):
        """Host-clock times (ms) of the last extract_stereo under set_profiling(True): the four phases of extract_times without
        the stereo tail, then the stereo tail."""
        ms = np.zeros(5, dtype=np.float64)
        capi.check(self.lib.osh_orb_extract_stereo_get_times(self.ctx, capi.ptr(ms, capi.c_double_p)), "osh_orb_extract_stereo_get_times", self.lib)
        return ms

    def _times(self, symbol):
        """Host-clock phases (ms) of an entry's last call under set_profiling(True): staging, upload, kernels, download."""
        ms = np.zeros(4, dtype=np.float64)
        capi.check(getattr(self.lib, symbol)(self.ctx, capi.ptr(ms, capi.c_double_p)), symbol, self.lib)
        return ms

    stereo_times = functools.partialmethod(_times, "osh_orb_stereo_get_times")                   # of the last stereo_match
    fisheye_stereo_times = functools.partialmethod(_times, "osh_orb_fisheye_stereo_get_times")   # of the last fisheye_stereo_match
    newpoint_times = functools.partialmethod(_times, "osh_orb_newpoint_get_times")               # of the last triangulate_new_points
    two_view_times = functools.partialmethod(_times, "osh_orb_two_view_get_times")               # of the last two_view_reconstruct
    refresh_map_points_times = functools.partialmethod(_times, "osh_orb_refresh_map_points_get_times")   # of the last refresh_map_points
    fast_times = functools.partialmethod(_times, "osh_orb_fast_get_times")                       # of the last fast_detect
    ic_angle_times = functools.partialmethod(_times, "osh_orb_ic_angle_get_times")               # of the last ic_angle
    describe_times = functools.partialmethod(_times, "osh_orb_describe_get_times")               # of the last describe
    bow_times = functools.partialmethod(_times, "osh_orb_bow_get_times")                         # of the last bow_transform
    bow_db_times = functools.partialmethod(_times, "osh_orb_bow_db_get_times")                   # of the last bow_db_query

    def bow_db_query(self, db: "BowDb", queries) -> list:
        """The inverted-file walk and the L1 scores of KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates
        for a batch of queries in one osh_orb_bow_db_query call.  A query is (word_id, value) or (word_id, value, excluded
        handles); per query a dict with max_common, min_common and, for the live rows that share a word, in ascending handle
        order: handle, common, first_word, scored, score."""
        cq, cr, _keep, outs = bow_db_args(queries, db.info()["live_rows"])
        capi.check(self.lib.osh_orb_bow_db_query(self.ctx, db.handle, len(queries), cq, cr), "osh_orb_bow_db_query", self.lib)
        return [bow_db_trim(o) for o in outs]

    def bow_transform(self, vocab: "BowVocab", frames, levelsup: int = 4, stages: bool = False) -> list:
        """TemplatedVocabulary::transform for a batch of descriptor arrays [n, 32] in one osh_orb_bow_transform call: per frame a
        dict with word_id / word_value (the BowVector) and node_id / node_start / node_feat (the FeatureVector as CSR), and with
        `stages` also feat_word, feat_node, feat_dist."""
        cf, cr, _keep, outs = bow_args(frames, stages)
        capi.check(self.lib.osh_orb_bow_transform(self.ctx, vocab.handle, int(levelsup), len(frames), cf, cr), "osh_orb_bow_transform", self.lib)
        return [bow_trim(o) for o in outs]

    def fisheye_stereo_match(self, frames, stages: bool = False) -> list:
        """Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1131-1171) for a batch of synth_fisheye.FisheyeFrame in one
        osh_orb_fisheye_stereo_match call: per frame a dict with left_to_right / right_to_left / depth / p3d [n, 3], and with
        `stages` also best_right, best_dist, second_dist, cos_parallax, stage."""
        cf, cr, _keep, outs = fisheye_stereo_args(frames, stages)
        capi.check(self.lib.osh_orb_fisheye_stereo_match(self.ctx, len(frames), cf, cr), "osh_orb_fisheye_stereo_match", self.lib)
        return outs

    def triangulate_new_points(self, segments) -> list:
        """The per-match body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:503-720) for a batch of
        synth_newpoints.Segment in one osh_orb_triangulate_new_points call: per segment a dict with stage, source,
        cos_parallax [n] and x3d [n, 3]."""
        cs, cr, _keep, outs = newpoint_args(segments)
        capi.check(self.lib.osh_orb_triangulate_new_points(self.ctx, len(segments), cs, cr), "osh_orb_triangulate_new_points", self.lib)
        return outs

    def two_view_reconstruct(self, problems, debug: bool = False) -> list:
        """TwoViewReconstruction::Reconstruct behind its minimal-set draw (src/TwoViewReconstruction.cc:100-129 and what it calls)
        for a batch of synth_two_view.Problem in one osh_orb_two_view_reconstruct call: per problem a dict with status, T21 [12],
        sh, sf, H21, F21 [3, 3], best_h, best_f, info [4], inlier, triangulated [n], x3d [n, 3], n_good, parallax [8], and with
        `debug` also debug_model_n, debug_model [2, iterations, 3, 3], debug_score [2, iterations], debug_R [8, 3, 3], debug_t [8, 3]."""
        cp, cr, _keep, outs = two_view_args(problems, debug)
        capi.check(self.lib.osh_orb_two_view_reconstruct(self.ctx, len(problems), cp, cr), "osh_orb_two_view_reconstruct", self.lib)
        return outs

    def mlpnp_solve(self, problems, debug: bool = False, fill=None) -> list:
        """MLPnPsolver::iterate behind its minimal-set draw (src/MLPnPsolver.cpp:100-353) for a batch of synth_mlpnp.Problem in one
        osh_orb_mlpnp_solve call: per problem a dict with first_hit, hit_record, hit_pose [12], hit_count, hit_mask [words],
        best_iteration, best_count, best_mask, best_pose, best_refine_ok, n_records, debug_count, debug_record, debug_record_count
        [iterations], and with `debug` also debug_pose and debug_record_pose [iterations, 12]."""
        cp, cr, _keep, outs = mlpnp_args(problems, debug, fill)
        capi.check(self.lib.osh_orb_mlpnp_solve(self.ctx, len(problems), cp, cr), "osh_orb_mlpnp_solve", self.lib)
        return outs

    def mlpnp_check_inliers(self, problem, poses):
        """CheckInliers (src/MLPnPsolver.cpp:262-293) of the poses [k, 12] against a synth_mlpnp.Problem's correspondences
        (osh_orb_mlpnp_check_inliers): count [k], mask [k, words]."""
        rc, count, mask = _ransac_check_inliers(lambda *a: self.lib.osh_orb_mlpnp_check_inliers(self.ctx, *a), mlpnp_args, problem, poses,
                                                np.float64, 12)
        capi.check(rc, "osh_orb_mlpnp_check_inliers", self.lib)
        return count, mask

    def mlpnp_times(self):
        """Phases (ms) of the last mlpnp_solve under set_profiling(True): staging, upload, kernels, download, and the hypothesis
        kernel alone (part of the kernels)."""
        ms = np.zeros(5, dtype=np.float64)
        capi.check(self.lib.osh_orb_mlpnp_get_times(self.ctx, capi.ptr(ms, capi.c_double_p)), "osh_orb_mlpnp_get_times", self.lib)
        return ms

    def sim3_ransac(self, problems, debug: bool = False, fill=None) -> list:
        """Sim3Solver::iterate behind its minimal-set draw (src/Sim3Solver.cc:149-294) for a batch of synth_sim3_ransac.Problem in
        one osh_orb_sim3_ransac call: per problem a dict with first_hit, n_records, record, record_count [iterations], record_T
        [iterations, 13], record_mask [iterations, words], best_iteration, best_count, debug_count [iterations], and with `debug`
        also debug_T [iterations, 13]."""
        cp, cr, _keep, outs = sim3_ransac_args(problems, debug, fill)
        capi.check(self.lib.osh_orb_sim3_ransac(self.ctx, len(problems), cp, cr), "osh_orb_sim3_ransac", self.lib)
        return outs

    def sim3_ransac_check_inliers(self, problem, T12s):
        """CheckInliers (src/Sim3Solver.cc:415-439) of the transforms [k, 13] (R, t, s) against a synth_sim3_ransac.Problem's
        correspondences (osh_orb_sim3_ransac_check_inliers): count [k], mask [k, words]."""
        rc, count, mask = _ransac_check_inliers(lambda *a: self.lib.osh_orb_sim3_ransac_check_inliers(self.ctx, *a), sim3_ransac_args, problem,
                                                T12s, np.float32, 13)
        capi.check(rc, "osh_orb_sim3_ransac_check_inliers", self.lib)
        return count, mask

    def sim3_ransac_times(self):
        """Phases (ms) of the last sim3_ransac under set_profiling(True): staging, upload, kernels, download."""
        ms = np.zeros(4, dtype=np.float64)
        capi.check(self.lib.osh_orb_sim3_ransac_get_times(self.ctx, capi.ptr(ms, capi.c_double_p)), "osh_orb_sim3_ransac_get_times", self.lib)
        return ms

    def refresh_map_points(self, batches, want=None) -> list:
        """MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth (src/MapPoint.cc:329-403,426-494) for a list of
        synth_mappoints.Batch in one osh_orb_refresh_map_points call: per batch a dict with best_entry, best_median [n],
        normal [n, 3], min_distance and max_distance [n].  want: the names of the outputs asked for (None: all)."""
        cb, cr, _keep, outs = mappoint_args(batches, want)
        capi.check(self.lib.osh_orb_refresh_map_points(self.ctx, len(batches), cb, cr), "osh_orb_refresh_map_points", self.lib)
        return outs

    def fuse_search(self, targets, points, mode: int = capi.OSH_FUSE_CHI2, fill=None) -> dict:
        """The search of ORBmatcher::Fuse (src/ORBmatcher.cc:1148-1455) for a list of synth_fuse.Target and one synth_fuse.Points in
        one osh_orb_fuse_search call: stage, u, v, ur, level, radius, n_candidates, best_idx, best_dist, each [n_targets, n]."""
        ct, cp, cr, _keep, out = fuse_args(targets, points, fill)
        capi.check(self.lib.osh_orb_fuse_search(self.ctx, len(targets), ct, C.byref(cp), mode, C.byref(cr)), "osh_orb_fuse_search", self.lib)
        return out

    fuse_times = functools.partialmethod(_times, "osh_orb_fuse_get_times")                       # of the last fuse_search

    def keyframe_cull_stage(self, problem):
        """Uploads a synth_keyframe_cull.CullProblem (osh_orb_keyframe_cull_stage): it stays resident until the next stage call."""
        cp, _keep = kfcull_problem(problem)
        capi.check(self.lib.osh_orb_keyframe_cull_stage(self.ctx, C.byref(cp)), "osh_orb_keyframe_cull_stage", self.lib)
        self._kfcull_candidates = int(problem.n_candidates)

    def keyframe_cull_count(self, removed=(), first_candidate: int = 0, n_candidates: int | None = None) -> dict:
        """nMPs, nRedundantObservations and the decision of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:976-1044) for the
        candidates from first_candidate on of the staged problem under a removed set (osh_orb_keyframe_cull_count)."""
        n = max(0, (self._kfcull_candidates if n_candidates is None else n_candidates) - first_candidate)
        out, cr = kfcull_result(n)
        rm = np.ascontiguousarray(removed, np.int32).reshape(-1)
        capi.check(self.lib.osh_orb_keyframe_cull_count(self.ctx, len(rm), capi.ptr(rm, capi.c_int32_p), int(first_candidate), C.byref(cr)),
                   "osh_orb_keyframe_cull_count", self.lib)
        return out

    keyframe_cull_times = functools.partialmethod(_times, "osh_orb_keyframe_cull_get_times")   # of the last stage and the last count

    def fast_detect(self, frames, capacities=None, borders=None) -> list:
        """The cell-wise FAST corners of ORBextractor::ComputeKeyPointsOctTree (src/ORBextractor.cc:787-872) for a batch of
        synth_fast.FastFrame in one osh_orb_fast_detect call: per frame a dict with n_out, n_cells, token, level_count and xy [n, 2],
        response, level, cell, used_min_th.  capacities: per frame (capacity, cell_capacity); a frame that does not fit comes back
        with its counts and None for the arrays.  None: a first call with no room sizes the arrays of a second."""
        if capacities is None:
            sized = self.fast_detect(frames, [(0, 0)] * len(frames), borders)
            capacities = [(r["n_out"], r["n_cells"]) for r in sized]
        cf, cr, _keep, outs = fast_args(frames, capacities, borders)
        capi.check(self.lib.osh_orb_fast_detect(self.ctx, len(frames), cf, cr), "osh_orb_fast_detect", self.lib)
        return _fast_outputs(cr, outs)

    def fast_detect_resident(self, items, capacities=None) -> list:
        """osh_orb_fast_detect over frames of the resident pyramid in one osh_orb_fast_detect_resident call: items are
        dict(token, n_levels, ini_th, min_th); the per-frame dicts and `capacities` are those of fast_detect."""
        if capacities is None:
            sized = self.fast_detect_resident(items, [(0, 0)] * len(items))
            capacities = [(r["n_out"], r["n_cells"]) for r in sized]
        cf, cr, _keep, outs = fast_resident_args(items, capacities)
        capi.check(self.lib.osh_orb_fast_detect_resident(self.ctx, len(items), cf, cr), "osh_orb_fast_detect_resident", self.lib)
        return _fast_outputs(cr, outs)

    def octree_distribute(self, lists, capacities=None) -> list:
        """ORBextractor::DistributeOctTree (src/ORBextractor.cc:480-779) for a batch of lists (xy [n, 2], response [n], width,
        height, n_features) in one osh_orb_octree_distribute call: per list a dict with n_out, status and index (the kept input
        indices in result order).  capacities: per list the room of index; a list that does not fit comes back with its count and
        None for the array.  None: room for every candidate."""
        cl, cr, _keep, outs = octree_args(lists, capacities)
        capi.check(self.lib.osh_orb_octree_distribute(self.ctx, len(lists), cl, cr), "osh_orb_octree_distribute", self.lib)
        return _octree_outputs(cr, outs)

    octree_times = functools.partialmethod(_times, "osh_orb_octree_get_times")                   # of the last octree_distribute

    def pyramid_build(self, items, download: bool = True) -> list:
        """ORBextractor::ComputePyramid (src/ORBextractor.cc:1170-1195) for a batch of items dict(image uint8 [rows, cols] (rows may
        be strided), inv_scale [n_levels], optionally border (19)) in one osh_orb_pyramid_build call: per item a dict with token,
        shapes [(rows, cols)] and, with `download`, levels (views into `bordered`, the whole images with the border around them)."""
        cf, cr, _keep, outs = pyramid_args(items, download)
        capi.check(self.lib.osh_orb_pyramid_build(self.ctx, len(items), cf, cr), "osh_orb_pyramid_build", self.lib)
        return _pyramid_outputs(cr, outs)

    pyramid_times = functools.partialmethod(_times, "osh_orb_pyramid_get_times")                 # of the last pyramid_build

    def ic_angle(self, items, borders=None) -> list:
        """IC_Angle (src/ORBextractor.cc:76-103) for a batch of items dict(xy, level, pyramid or token) in one osh_orb_ic_angle
        call: per item a dict with angle, m10, m01."""
        cf, cr, _keep, outs = ic_angle_args(items, borders)
        capi.check(self.lib.osh_orb_ic_angle(self.ctx, len(items), cf, cr), "osh_orb_ic_angle", self.lib)
        return outs

    def describe(self, items, borders=None, debug: bool = False) -> list:
        """The blur and the steered-BRIEF descriptors of ORBextractor::operator() (src/ORBextractor.cc:1123-1165) for a batch of
        items dict(xy, level, angle, pattern [512, 2] int8, pyramid or token, optionally blur_q8 [7]) in one osh_orb_describe call:
        per item a dict with descriptors [n, 32], and with `debug` also cos_sin [n, 2] and blurred (the blurred levels as a list;
        an item by token then names its level shapes under `shapes`)."""
        cf, cr, _keep, outs = describe_args(items, borders, debug)
        capi.check(self.lib.osh_orb_describe(self.ctx, len(items), cf, cr), "osh_orb_describe", self.lib)
        return _describe_outputs(outs)

    describe_cpu = staticmethod(lambda items, borders=None, debug=False: describe_cpu(items, borders=borders, debug=debug))

    def extract(self, items, capacities=None, download: bool = False) -> list:
        """ORBextractor::operator() up to its write-back for a batch of items dict(image, inv_scale, scale, n_features [n_levels],
        pattern [512, 2] int8, optionally ini_th (20), min_th (7), blur_q8 [7], border (19)) in ONE osh_orb_extract call: per item a
        dict with n_out, token, level_count and xy [n, 2] (level pixels), level, response, angle, size, descriptors [n, 32] (None
        when the arrays were too small), and with `download` also levels / bordered as pyramid_build gives them.  capacities: per
        item the room of the arrays; None: a first call with no room sizes them."""
        if capacities is None:
            capacities = [r["n_out"] for r in self.extract(items, [0] * len(items))]
        cf, cr, _keep, outs = extract_args(items, capacities, download)
        capi.check(self.lib.osh_orb_extract(self.ctx, len(items), cf, cr), "osh_orb_extract", self.lib)
        return _extract_outputs(cr, outs)

    extract_times = functools.partialmethod(_times, "osh_orb_extract_get_times")                 # of the last extract or extract_raw

    def rectify_map(self, map_x, map_y, src_shape) -> "RectifyMap":
        """A rectify map (osh_rectify_map) resident on this matcher's device from the float32 maps [rows, cols] (rows may be strided)
        and the (rows, cols) of the images it was made for; the caller closes it."""
        return RectifyMap(map_x, map_y, src_shape, self.device)

    def prepare(self, items, download: bool = True) -> list:
        """The image front end (remap or resize, then grey) for a batch of items dict(image uint8 [rows, cols] or [rows, cols, 3 | 4]
        (rows may be strided), optionally order ("rgb" / "bgr"), map (a RectifyMap), out_shape (rows, cols)) in one osh_orb_prepare
        call: per item a dict with shape and, with `download`, gray (a view into `gray_whole`, whose rows are longer)."""
        cf, cr, _maps, _keep, outs = prepare_args(items, download)
        capi.check(self.lib.osh_orb_prepare(self.ctx, len(items), cf, cr), "osh_orb_prepare", self.lib)
        return _prepare_outputs(cr, outs)

    prepare_times = functools.partialmethod(_times, "osh_orb_prepare_get_times")                 # of the last prepare

    def extract_raw(self, items, capacities=None, download: bool = False, gray: bool = False) -> list:
        """extract() on raw images in ONE osh_orb_extract_raw call: items carry the keys of prepare() and of extract() (image being
        the raw one).  Per item the dict of extract(), and with `gray` also gray and shape as prepare() gives them."""
        if capacities is None:
            capacities = [r["n_out"] for r in self.extract_raw(items, [0] * len(items))]
        pf, pr, _maps, _pkeep, pouts = prepare_args(items, gray)
        cf, cr, _keep, outs = extract_raw_args(items, capacities, download)
        capi.check(self.lib.osh_orb_extract_raw(self.ctx, len(items), pf, cf, cr, pr if gray else None), "osh_orb_extract_raw", self.lib)
        res = _extract_outputs(cr, outs)
        if gray:
            for d, p in zip(res, _prepare_outputs(pr, pouts)):
                d.update(p)
        return res

    def kb8_triangulate(self, rig: "capi.Kb8Rig", xy1, xy2, sigma1, sigma2) -> dict:
        """KannalaBrandt8::TriangulateMatches for explicit keypoint pairs (osh_kb8_triangulate): ret [n], p3d [n, 3], cos_parallax [n]."""
        a = kb8_pairs(xy1, xy2, sigma1, sigma2)
        n = a[0].shape[0]
        out = dict(ret=np.zeros(n, np.float32), p3d=np.zeros((n, 3), np.float32), cos_parallax=np.zeros(n, np.float32))
        capi.check(self.lib.osh_kb8_triangulate(self.ctx, n, C.byref(rig), *[capi.ptr(x, capi.c_float_p) for x in a],
                                                capi.ptr(out["ret"], capi.c_float_p), capi.ptr(out["p3d"], capi.c_float_p),
                                                capi.ptr(out["cos_parallax"], capi.c_float_p)), "osh_kb8_triangulate", self.lib)
        return out

    def set_profiling(self, enable: bool):
        capi.check(self.lib.osh_orb_set_profiling(self.ctx, int(enable)), "osh_orb_set_profiling", self.lib)

    def profile(self):
        n, ms = C.c_int64(0), C.c_double(0)
        capi.check(self.lib.osh_orb_get_profile(self.ctx, C.byref(n), C.byref(ms)), "osh_orb_get_profile", self.lib)
        return int(n.value), float(ms.value)


    def resolve_profile(self):
        n, ms = C.c_int64(0), C.c_double(0)
        capi.check(self.lib.osh_orb_get_resolve_profile(self.ctx, C.byref(n), C.byref(ms)), "osh_orb_get_resolve_profile", self.lib)
        return int(n.value), float(ms.value)


class BowVocab:
    """A device-resident vocabulary (osh_bow_vocab) made from a synth_bow.BowTree; shared by every OrbMatcher of the device."""

    def __init__(self, tree, device: int = 0):
        self.lib = capi.load_library()
        self.handle = C.c_void_p()
        t, _keep = bow_tree(tree)
        capi.check(self.lib.osh_bow_vocab_create(device, C.byref(t), C.byref(self.handle)), "osh_bow_vocab_create", self.lib)

    def close(self):
        if self.handle:
            self.lib.osh_bow_vocab_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RectifyMap:
    """The float32 maps of a camera and the source size they were made for; with a device, resident there as an osh_rectify_map and
    shared by every OrbMatcher of the device.  device None: the description alone, for prepare_cpu."""

    def __init__(self, map_x, map_y, src_shape, device: int | None = None):
        self.map_x, self.map_y = np.asarray(map_x), np.asarray(map_y)
        for m in (self.map_x, self.map_y):
            assert m.dtype == np.float32 and m.ndim == 2 and m.shape == self.map_x.shape and (m.shape[1] == 1 or m.strides[1] == 4)
        self.src_shape = (int(src_shape[0]), int(src_shape[1]))
        self.shape = tuple(self.map_x.shape)
        self.handle = C.c_void_p()
        self.lib = None
        if device is not None:
            self.lib = capi.load_library()
            d = self.desc()
            capi.check(self.lib.osh_rectify_map_create(device, C.byref(d), C.byref(self.handle)), "osh_rectify_map_create", self.lib)

    def desc(self) -> "capi.RectifyMapDesc":
        """The osh_rectify_map_desc; it points into this object's arrays."""
        d = capi.RectifyMapDesc()
        d.rows, d.cols = self.shape
        d.src_rows, d.src_cols = self.src_shape
        d.map_x, d.map_y = C.cast(self.map_x.ctypes.data, capi.c_float_p), C.cast(self.map_y.ctypes.data, capi.c_float_p)
        d.map_x_stride = self.map_x.strides[0] if self.shape[0] > 1 else max(self.map_x.strides[0], 4 * self.shape[1])
        d.map_y_stride = self.map_y.strides[0] if self.shape[0] > 1 else max(self.map_y.strides[0], 4 * self.shape[1])
        return d

    def close(self):
        if self.handle:
            self.lib.osh_rectify_map_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BowDb:
    """A device-resident, mutable database of BowVectors (osh_bow_db) over a vocabulary of n_words words; queried through
    OrbMatcher.bow_db_query by any number of matchers of the device at once."""

    INFO = ("live_rows", "rows", "entries", "capacity", "compactions", "reallocations")

    def __init__(self, n_words: int, device: int = 0):
        self.lib = capi.load_library()
        self.handle = C.c_void_p()
        capi.check(self.lib.osh_bow_db_create(device, int(n_words), C.byref(self.handle)), "osh_bow_db_create", self.lib)

    def close(self):
        if self.handle:
            self.lib.osh_bow_db_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, word_id, value) -> int:
        """A new last row; its handle."""
        w, v = np.ascontiguousarray(word_id, np.int32), np.ascontiguousarray(value, np.float64)
        assert w.shape == v.shape and w.ndim == 1
        h = C.c_uint64(0)
        capi.check(self.lib.osh_bow_db_add(self.handle, w.shape[0], capi.ptr(w, capi.c_int32_p), capi.ptr(v, capi.c_double_p), C.byref(h)),
                   "osh_bow_db_add", self.lib)
        return int(h.value)

    def erase(self, handle: int):
        capi.check(self.lib.osh_bow_db_erase(self.handle, int(handle)), "osh_bow_db_erase", self.lib)

    def clear(self):
        capi.check(self.lib.osh_bow_db_clear(self.handle), "osh_bow_db_clear", self.lib)

    def info(self) -> dict:
        a = np.zeros(6, np.int64)
        capi.check(self.lib.osh_bow_db_info(self.handle, capi.ptr(a, capi.c_int64_p)), "osh_bow_db_info", self.lib)
        return dict(zip(self.INFO, (int(x) for x in a)))


_POINTER = {np.dtype(np.float32): capi.c_float_p, np.dtype(np.int32): capi.c_int32_p, np.dtype(np.uint8): capi.c_uint8_p,
            np.dtype(np.float64): capi.c_double_p, np.dtype(np.uint64): C.POINTER(C.c_uint64), np.dtype(np.uint32): capi.c_uint32_p}
# the keypoint arrays of a frame: attribute of the synthetic frame = field of the frame struct, key in the dict of arrays, dtype
_KEYPOINTS = (("left_xy", "lxy", np.float32), ("left_octave", "loct", np.int32), ("left_desc", "ldesc", np.uint8),
              ("right_xy", "rxy", np.float32), ("right_octave", "roct", np.int32), ("right_desc", "rdesc", np.uint8))


def _fill_keypoints(f, fr, a=None):
    """n_left, n_right and the six keypoint arrays of a capi.StereoFrame, capi.FisheyeStereoFrame or capi.HostFisheyeInput from a
    synthetic frame; a: its contiguous arrays if the caller made them already.  Returns the arrays the pointers refer to."""
    if a is None:
        a = {key: np.ascontiguousarray(getattr(fr, field), dtype) for field, key, dtype in _KEYPOINTS}
    f.n_left, f.n_right = a["loct"].shape[0], a["roct"].shape[0]
    for field, key, _ in _KEYPOINTS:
        setattr(f, field, capi.ptr(a[key], _POINTER[a[key].dtype]))
    return a


def _wire_outputs(res, outs):
    """Points the fields of a result struct at the arrays of `outs` (field name -> array), each through the pointer type of its dtype."""
    for name, o in outs.items():
        setattr(res, name, capi.ptr(o, _POINTER[o.dtype]))


def _bordered_image(im, rows, cols, border):
    """A whole image of 167 with `border` pixels around a level of rows x cols, and `im` (a capi.StereoImage or capi.PyramidImage)
    set to the level as a view into it.  Returns the whole image and the level."""
    whole = np.full((max(rows, 0) + 2 * border, max(cols, 0) + 2 * border), 167, np.uint8)
    im.data = C.cast(whole.ctypes.data + border * whole.shape[1] + border, capi.c_uint8_p)
    im.rows, im.cols, im.stride = rows, cols, whole.shape[1]
    return whole, whole[border:border + rows, border:border + cols]


def pyramid_images(levels, border, keep: dict):
    """The osh_stereo_image array of a pyramid (a list of uint8 [rows, cols] arrays; None: the level's data stays NULL), every level
    handed over as a view into an image with `border` pixels of 167 around it.  The images are added to `keep`."""
    imgs = (capi.StereoImage * max(len(levels), 1))()
    for l, m in enumerate(levels):
        if m is None:
            continue
        keep[f"img{len(keep)}"], level = _bordered_image(imgs[l], m.shape[0], m.shape[1], border)
        level[:] = m
    return imgs


def _fill_pyramid_or_token(f, it, border, keep: dict):
    """The pyramid of an osh_ic_angle_frame or osh_describe_frame: brought along (it["pyramid"], a list of levels) or, without one,
    resident under it["token"]."""
    if it.get("pyramid") is not None:
        f.n_levels = len(it["pyramid"])
        f.pyramid = keep["pyr"] = pyramid_images(list(it["pyramid"]), border, keep)
    else:
        f.pyramid_token = int(it["token"])


def cut_levels(flat, shapes, copy: bool = True) -> list:
    """Flat pixels cut into levels of the given (rows, cols), one after the other; views into `flat` without `copy`."""
    levels, off = [], 0
    for r, c in shapes:
        level = flat[off:off + r * c].reshape(r, c)
        levels.append(level.copy() if copy else level)
        off += r * c
    return levels


def counted_call(fn, name, cin, out_type, second, arrays, needed):
    """A wrapper of the test library whose first pass counts: arrays(capacity, second capacity) makes the output arrays, which go
    into an out_type with the two capacities (the fields `capacity` and `second`), and needed(n, o) says what the pass with the
    return value n asked for.  At most two passes; returns n and the arrays of the pass that had the room."""
    caps = (0, 0)
    for _ in range(2):
        o = arrays(*caps)
        cout = out_type(capacity=caps[0], **{second: caps[1]})
        _wire_outputs(cout, o)
        n = fn(C.byref(cin), C.byref(cout))
        if n < 0:
            raise RuntimeError(f"{name} returned {n}")
        need = needed(n, o)
        if need[0] <= caps[0] and need[1] <= caps[1]:
            break
        caps = need
    return n, o


def fill_host_extract_input(cin, image, nfeatures, scale_factor, nlevels, ini_th, min_th, lapping=(0, 0)):
    """A capi.HostExtractInput from the stand-in constructor's arguments and a uint8 image (None or an empty array: an empty image).
    Returns the array `pixels` points to."""
    img = np.zeros((0, 0), np.uint8) if image is None else np.ascontiguousarray(image, np.uint8)
    cin.nfeatures, cin.scale_factor, cin.nlevels, cin.ini_th, cin.min_th = int(nfeatures), float(scale_factor), int(nlevels), int(ini_th), int(min_th)
    cin.rows, cin.cols = (img.shape if img.size else (0, 0))
    cin.pixels = capi.ptr(img if img.size else None, capi.c_uint8_p)
    cin.lapping[0], cin.lapping[1] = int(lapping[0]), int(lapping[1])
    return img


def stereo_args(frames, stages: bool = False, borders=None):
    """The osh_stereo_frame / osh_stereo_result arrays of OrbMatcher.stereo_match for repeated calls: (frames, results, the arrays
    that keep their pointers alive, the per-frame dicts of output arrays)."""
    n_frames = len(frames)
    cf = (capi.StereoFrame * max(n_frames, 1))()
    cr = (capi.StereoResult * max(n_frames, 1))()
    keep, outs = [], []
    for k, fr in enumerate(frames):
        border = 0 if borders is None else int(borders[k])
        f = cf[k]
        a = _fill_keypoints(f, fr)
        a.update(sf=np.ascontiguousarray(fr.scale_factors, np.float32), isf=np.ascontiguousarray(fr.inv_scale_factors, np.float32))
        f.n_levels = fr.n_levels
        f.scale_factors, f.inv_scale_factors = capi.ptr(a["sf"], capi.c_float_p), capi.ptr(a["isf"], capi.c_float_p)
        pyr = []
        for side in (fr.left_pyramid, fr.right_pyramid):
            pyr.append(pyramid_images(side, border, a))
        f.left_pyramid, f.right_pyramid = pyr[0], pyr[1]
        f.bf, f.b = fr.bf, fr.b
        n = f.n_left
        o = dict(u_right=np.zeros(n, np.float32), depth=np.zeros(n, np.float32))
        if stages:
            o.update(best_right=np.zeros(n, np.int32), hamming=np.zeros(n, np.int32), sad=np.zeros((n, 11), np.int32),
                     best_inc=np.zeros(n, np.int32), stage=np.zeros(n, np.uint8))
        _wire_outputs(cr[k], o)
        keep.append((a, pyr))
        outs.append(o)
    return cf, cr, keep, outs


def _stereo_result(res, n, stages: bool) -> dict:
    """The output arrays of an osh_stereo_result for n left keypoints, wired into `res`."""
    o = dict(u_right=np.zeros(n, np.float32), depth=np.zeros(n, np.float32))
    if stages:
        o.update(best_right=np.zeros(n, np.int32), hamming=np.zeros(n, np.int32), sad=np.zeros((n, 11), np.int32),
                 best_inc=np.zeros(n, np.int32), stage=np.zeros(n, np.uint8))
    _wire_outputs(res, o)
    return o


def stereo_resident_args(frames, tokens, stages: bool = False):
    """The osh_stereo_resident_frame / osh_stereo_result arrays of OrbMatcher.stereo_match_resident: stereo_args without the
    pyramids, tokens[k] = (left_token, right_token) in their place."""
    n_frames = len(frames)
    cf = (capi.StereoResidentFrame * max(n_frames, 1))()
    cr = (capi.StereoResult * max(n_frames, 1))()
    keep, outs = [], []
    for k, fr in enumerate(frames):
        f = cf[k]
        a = _fill_keypoints(f, fr)
        a.update(sf=np.ascontiguousarray(fr.scale_factors, np.float32), isf=np.ascontiguousarray(fr.inv_scale_factors, np.float32))
        f.n_levels = fr.n_levels
        f.scale_factors, f.inv_scale_factors = capi.ptr(a["sf"], capi.c_float_p), capi.ptr(a["isf"], capi.c_float_p)
        f.left_token, f.right_token = int(tokens[k][0]), int(tokens[k][1])
        f.bf, f.b = fr.bf, fr.b
        keep.append(a)
        outs.append(_stereo_result(cr[k], f.n_left, stages))
    return cf, cr, keep, outs


def extract_stereo_args(pairs, capacities, download: bool = False, stages: bool = False, raw: bool = False):
    """The arrays of OrbMatcher.extract_stereo for pairs dict(left, right, bf, b) (left / right: items of extract, or of extract_raw
    with `raw`) and the capacities of the 2 n frames: (prepare frames or None, extract frames, pairs, extract results, stereo
    results, keep-alive, per-frame extract outputs, per-pair stereo outputs)."""
    items = [it for p in pairs for it in (p["left"], p["right"])]
    pf, pkeep = None, None
    if raw:
        pf, _pr, _maps, pkeep, _pouts = prepare_args(items, False)
        cf, cr, keep, outs = extract_raw_args(items, capacities, download)
    else:
        cf, cr, keep, outs = extract_args(items, capacities, download)
    cp = (capi.StereoPair * max(len(pairs), 1))()
    cs = (capi.StereoResult * max(len(pairs), 1))()
    souts = []
    for p, pair in enumerate(pairs):
        cp[p].bf, cp[p].b = float(pair["bf"]), float(pair["b"])
        souts.append(_stereo_result(cs[p], int(capacities[2 * p]), stages))
    return pf, cf, cp, cr, cs, (keep, pkeep, _maps if raw else None), outs, souts


def _extract_stereo_outputs(cr, outs, souts):
    """Per pair: left / right as _extract_outputs gives them, and stereo: the arrays cut to the left count, None when either frame
    did not fit (stereo_arrays: the arrays as they were handed over)."""
    ex = _extract_outputs(cr, outs)
    res = []
    for p, so in enumerate(souts):
        left, right = ex[2 * p], ex[2 * p + 1]
        fits = left["xy"] is not None and right["xy"] is not None
        res.append(dict(left=left, right=right, stereo={name: v[:left["n_out"]] for name, v in so.items()} if fits else None, stereo_arrays=so))
    return res


def fast_level_cells(rows, cols, host_lib=None):
    """The cell geometry of csrc/orb_fast.h on the host (osh_host_orb_fast_level_cells of the test library): (nCols, nRows, wCell,
    hCell, maxBorderX, maxBorderY) and the [n, 4] rectangles x0 y0 w h of the level's cells in (i, j) order."""
    host_lib = host_lib or capi.load_host_library()
    geom = np.zeros(6, np.int32)
    if host_lib.osh_host_orb_fast_level_cells(int(rows), int(cols), capi.ptr(geom, capi.c_int32_p), None) < 0:
        raise RuntimeError("osh_host_orb_fast_level_cells refused the level")
    rects = np.zeros((max(int(geom[0]) * int(geom[1]), 1), 4), np.int32)
    n = host_lib.osh_host_orb_fast_level_cells(int(rows), int(cols), capi.ptr(geom, capi.c_int32_p), capi.ptr(rects, capi.c_int32_p))
    return tuple(int(g) for g in geom), rects[:n].copy()


def _fast_result(res, n_levels, capacity):
    """The output arrays of an osh_fast_result for a (capacity, cell_capacity), wired into `res`."""
    cap, cell_cap = (int(c) for c in capacity)
    o = dict(level_count=np.zeros(n_levels, np.int32), xy=np.zeros((cap, 2), np.float32), response=np.zeros(cap, np.float32),
             level=np.zeros(cap, np.int32), cell=np.zeros(cap, np.int32), used_min_th=np.zeros(cell_cap, np.uint8))
    res.capacity, res.cell_capacity = cap, cell_cap
    _wire_outputs(res, o)
    return o


def fast_args(frames, capacities, borders=None):
    """The osh_fast_frame / osh_fast_result arrays of OrbMatcher.fast_detect for frames with .pyramid / .ini_th / .min_th
    (synth_fast.FastFrame) and per frame a (capacity, cell_capacity): (frames, results, keep-alive, per-frame dicts of outputs)."""
    n_frames = len(frames)
    cf = (capi.FastFrame * max(n_frames, 1))()
    cr = (capi.FastResult * max(n_frames, 1))()
    keep, outs = [], []
    for k, fr in enumerate(frames):
        a = {}
        cf[k].n_levels = len(fr.pyramid)
        cf[k].pyramid = pyramid_images(list(fr.pyramid), 0 if borders is None else int(borders[k]), a)
        a["pyr"] = cf[k].pyramid
        cf[k].ini_th, cf[k].min_th = int(fr.ini_th), int(fr.min_th)
        keep.append(a)
        outs.append(_fast_result(cr[k], len(fr.pyramid), capacities[k]))
    return cf, cr, keep, outs


def _fast_outputs(cr, outs):
    """Per frame: the counts, the token and, when the arrays were large enough, the arrays cut to their lengths (else None)."""
    res = []
    for k, o in enumerate(outs):
        n, nc = int(cr[k].n_out), int(cr[k].n_cells)
        d = dict(n_out=n, n_cells=nc, token=int(cr[k].pyramid_token), level_count=o["level_count"])
        fits = n <= int(cr[k].capacity) and nc <= int(cr[k].cell_capacity)
        for name in ("xy", "response", "level", "cell"):
            d[name] = o[name][:n] if fits else None
        d["used_min_th"] = o["used_min_th"][:nc] if fits else None
        res.append(d)
    return res


def octree_args(lists, capacities=None, counts=None):
    """The osh_octree_list / osh_octree_result arrays of OrbMatcher.octree_distribute for lists (xy, response, width, height,
    n_features) and per list the room of its index array (None: its candidate count): (lists, results, keep-alive, index arrays).
    counts: per list the candidate count to hand over whatever the arrays hold (for the refusals); xy and response may be None."""
    n_lists = len(lists)
    cl = (capi.OctreeList * max(n_lists, 1))()
    cr = (capi.OctreeResult * max(n_lists, 1))()
    keep, outs = [], []
    for k, (xy, response, width, height, n_features) in enumerate(lists):
        xy = None if xy is None else np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        response = None if response is None else np.ascontiguousarray(response, np.float32).reshape(-1)
        n = 0 if response is None else len(response)
        cl[k].n = n if counts is None else int(counts[k])
        cl[k].xy = None if xy is None else capi.ptr(xy, capi.c_float_p)
        cl[k].response = None if response is None else capi.ptr(response, capi.c_float_p)
        cl[k].width, cl[k].height, cl[k].n_features = int(width), int(height), int(n_features)
        cap = n if capacities is None else int(capacities[k])
        index = np.full(max(cap, 0), -1, np.int32)
        cr[k].capacity = cap
        cr[k].index = capi.ptr(index, capi.c_int32_p) if cap > 0 else None
        keep.append((xy, response))
        outs.append(index)
    return cl, cr, keep, outs


def _octree_outputs(cr, outs):
    """Per list: the count, the status and, when the array was large enough, the kept indices (else None)."""
    return [dict(n_out=int(cr[k].n_out), status=int(cr[k].status), index=o[:int(cr[k].n_out)] if 0 <= int(cr[k].n_out) <= int(cr[k].capacity) else None)
            for k, o in enumerate(outs)]


def octree_cpu(lists, capacities=None, host_lib=None, counts=None):
    """csrc/orb_octree.h on the host in one thread (osh_host_orb_octree_cpu of the test library): the per-list dicts of
    OrbMatcher.octree_distribute, the return code (the checks are those of the device call) and the wall time of the lists in ms."""
    host_lib = host_lib or capi.load_host_library()
    ms = C.c_double(0)
    cl, cr, _keep, outs = octree_args(lists, capacities, counts)
    rc = host_lib.osh_host_orb_octree_cpu(len(lists), cl, cr, C.byref(ms))
    return _octree_outputs(cr, outs), int(rc), float(ms.value)


def fast_resident_args(items, capacities):
    """The osh_fast_resident_frame / osh_fast_result arrays of OrbMatcher.fast_detect_resident for items dict(token, n_levels,
    ini_th, min_th) and per item a (capacity, cell_capacity)."""
    n = len(items)
    cf = (capi.FastResidentFrame * max(n, 1))()
    cr = (capi.FastResult * max(n, 1))()
    outs = []
    for k, it in enumerate(items):
        cf[k].pyramid_token, cf[k].ini_th, cf[k].min_th = int(it["token"]), int(it["ini_th"]), int(it["min_th"])
        outs.append(_fast_result(cr[k], int(it["n_levels"]), capacities[k]))
    return cf, cr, outs, outs


def pyramid_level_shapes(rows, cols, inv_scale) -> list:
    """(rows, cols) of every level as ORBextractor::ComputePyramid sizes them: cvRound((float)size * inv_scale[l]), halves to even."""
    inv = np.asarray(inv_scale, np.float32)
    return [(int(np.rint(np.float32(rows) * s)), int(np.rint(np.float32(cols) * s))) for s in inv]


def pyramid_args(items, download: bool = True):
    """The osh_pyramid_frame / osh_pyramid_result arrays of OrbMatcher.pyramid_build for items dict(image, inv_scale, optionally
    border): (frames, results, keep-alive, per-item dicts of outputs).  The image is read in place: a view with strided rows stays
    one.  With `download` every level gets a whole image of 167 with `border` pixels around the level."""
    n = len(items)
    cf = (capi.PyramidFrame * max(n, 1))()
    cr = (capi.PyramidResult * max(n, 1))()
    keep, outs = [], []
    for k, it in enumerate(items):
        img = it["image"]
        assert img.dtype == np.uint8 and img.ndim == 2 and (img.shape[1] == 1 or img.strides[1] == 1)
        inv = np.ascontiguousarray(it["inv_scale"], np.float32)
        nl = inv.shape[0]
        f = cf[k]
        f.image.data = C.cast(img.ctypes.data, capi.c_uint8_p)
        f.image.rows, f.image.cols, f.image.stride = img.shape[0], img.shape[1], img.strides[0] if img.shape[0] > 1 else max(img.strides[0], img.shape[1])
        f.n_levels, f.inv_scale = nl, capi.ptr(inv, capi.c_float_p)
        a = dict(img=img, inv=inv, level_rows=np.zeros(nl, np.int32), level_cols=np.zeros(nl, np.int32))
        cr[k].level_rows, cr[k].level_cols = capi.ptr(a["level_rows"], capi.c_int32_p), capi.ptr(a["level_cols"], capi.c_int32_p)
        o = dict(level_rows=a["level_rows"], level_cols=a["level_cols"])
        if download:
            b = int(it.get("border", 19))
            shapes = pyramid_level_shapes(img.shape[0], img.shape[1], inv)
            lv = (capi.PyramidImage * max(nl, 1))()
            o["bordered"], o["levels"] = [], []
            for l, (r, c) in enumerate(shapes):
                whole, level = _bordered_image(lv[l], r, c, b)
                o["bordered"].append(whole)
                o["levels"].append(level)
            a["lv"] = lv
            cr[k].levels, cr[k].border = lv, b
        keep.append(a)
        outs.append(o)
    return cf, cr, keep, outs


def _pyramid_outputs(cr, outs):
    res = []
    for k, o in enumerate(outs):
        d = dict(o, token=int(cr[k].pyramid_token), shapes=list(zip(o["level_rows"].tolist(), o["level_cols"].tolist())))
        res.append(d)
    return res


def extract_args(items, capacities, download: bool = False):
    """The osh_extract_frame / osh_extract_result arrays of OrbMatcher.extract: (frames, results, keep-alive, per-item outputs)."""
    n = len(items)
    pf, pr, pkeep, pouts = pyramid_args(items, download)
    cf = (capi.ExtractFrame * max(n, 1))()
    cr = (capi.ExtractResult * max(n, 1))()
    keep, outs = [pkeep], []
    for k, it in enumerate(items):
        nl = int(pf[k].n_levels)
        a = dict(scale=np.ascontiguousarray(it["scale"], np.float32), n_features=np.ascontiguousarray(it["n_features"], np.int32),
                 pattern=np.ascontiguousarray(it["pattern"], np.int8), blur=None if it.get("blur_q8") is None else np.ascontiguousarray(it["blur_q8"], np.uint16))
        f = cf[k]
        f.image, f.n_levels, f.inv_scale = pf[k].image, nl, pf[k].inv_scale
        f.scale, f.n_features = capi.ptr(a["scale"], capi.c_float_p), capi.ptr(a["n_features"], capi.c_int32_p)
        f.ini_th, f.min_th = int(it.get("ini_th", 20)), int(it.get("min_th", 7))
        f.pattern, f.blur_q8 = capi.ptr(a["pattern"], C.POINTER(C.c_int8)), capi.ptr(a["blur"], C.POINTER(C.c_uint16))
        cap = int(capacities[k])
        o = dict(level_count=np.zeros(nl, np.int32), xy=np.zeros((cap, 2), np.float32), level=np.zeros(cap, np.int32), response=np.zeros(cap, np.float32),
                 angle=np.zeros(cap, np.float32), size=np.zeros(cap, np.float32), descriptors=np.zeros((cap, 32), np.uint8))
        cr[k].capacity = cap
        _wire_outputs(cr[k], o)
        cr[k].levels, cr[k].border = pr[k].levels, pr[k].border
        o.update({name: pouts[k][name] for name in ("levels", "bordered") if name in pouts[k]})
        keep.append(a)
        outs.append(o)
    return cf, cr, keep, outs


def _extract_outputs(cr, outs):
    """Per item: the counts, the token and, when the arrays were large enough, the arrays cut to their lengths (else None)."""
    res = []
    for k, o in enumerate(outs):
        n = int(cr[k].n_out)
        d = dict(n_out=n, token=int(cr[k].pyramid_token), level_count=o["level_count"])
        for name in ("xy", "level", "response", "angle", "size", "descriptors"):
            d[name] = o[name][:n] if n <= int(cr[k].capacity) else None
        d.update({name: o[name] for name in ("levels", "bordered") if name in o})
        res.append(d)
    return res


def prepared_shape(it) -> tuple:
    """(rows, cols) of the image a prepare item gives: the map's size, else out_shape, else the input's."""
    if it.get("map") is not None:
        return tuple(it["map"].shape)
    if it.get("out_shape") is not None:
        return (int(it["out_shape"][0]), int(it["out_shape"][1]))
    return tuple(it["image"].shape[:2])


def prepare_args(items, download: bool = True):
    """The osh_prepare_frame / osh_prepare_result arrays of OrbMatcher.prepare: (frames, results, the host descriptors of the maps
    for prepare_cpu, keep-alive, per-item dicts of outputs).  The image is read in place: a view with strided rows stays one.  With
    `download` every result names a view into an image of 167 whose rows are 5 bytes longer."""
    n = len(items)
    cf = (capi.PrepareFrame * max(n, 1))()
    cr = (capi.PrepareResult * max(n, 1))()
    maps = (C.POINTER(capi.RectifyMapDesc) * max(n, 1))()
    keep, outs = [], []
    for k, it in enumerate(items):
        img = it["image"]
        ch = 1 if img.ndim == 2 else img.shape[2]
        assert img.dtype == np.uint8 and img.ndim in (2, 3) and (img.ndim == 2 or img.strides[2] == 1) and (img.shape[1] == 1 or img.strides[1] == ch)
        f = cf[k]
        f.image.data = C.cast(img.ctypes.data, capi.c_uint8_p)
        f.image.rows, f.image.cols, f.image.channels = img.shape[0], img.shape[1], ch
        f.image.stride = img.strides[0] if img.shape[0] > 1 else max(img.strides[0], img.shape[1] * ch)
        order = it.get("order", "rgb")
        f.order = {"rgb": capi.OSH_PREP_RGB, "bgr": capi.OSH_PREP_BGR}.get(order, order)
        a = dict(img=img)
        m = it.get("map")
        if m is not None:
            f.map = m.handle.value
            a["desc"] = m.desc()
            maps[k] = C.pointer(a["desc"])
        if it.get("out_shape") is not None:
            f.out_rows, f.out_cols = int(it["out_shape"][0]), int(it["out_shape"][1])
        o = {}
        if download:
            rows, cols = prepared_shape(it)
            o["gray_whole"] = np.full((max(rows, 0), max(cols, 0) + 5), 167, np.uint8)
            o["gray"] = o["gray_whole"][:, :max(cols, 0)]
            cr[k].gray, cr[k].gray_stride = C.cast(o["gray_whole"].ctypes.data, capi.c_uint8_p), o["gray_whole"].shape[1]
        keep.append(a)
        outs.append(o)
    return cf, cr, maps, keep, outs


def _prepare_outputs(cr, outs):
    return [dict(o, shape=(int(cr[k].rows), int(cr[k].cols))) for k, o in enumerate(outs)]


def prepare_cpu(items, host_lib=None):
    """csrc/orb_prepare.h on the host in one thread (osh_host_orb_prepare_cpu of the test library): the per-item dicts of
    OrbMatcher.prepare and the wall time of the loops in ms.  A map may be a RectifyMap without a device."""
    host_lib = host_lib or capi.load_host_library()
    ms = C.c_double(0)
    cf, cr, maps, _keep, outs = prepare_args(items, True)
    for k in range(len(items)):
        cf[k].map = None   # the host build reads the descriptor
    rc = host_lib.osh_host_orb_prepare_cpu(len(items), cf, maps, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_orb_prepare_cpu -> {rc}")
    return _prepare_outputs(cr, outs), float(ms.value)


def extract_raw_args(items, capacities, download: bool = False):
    """The osh_extract_frame / osh_extract_result arrays of OrbMatcher.extract_raw: those of extract_args for an image of the
    prepared size that brings no data."""
    sized = [dict(it, image=np.empty(prepared_shape(it), np.uint8)) for it in items]
    cf, cr, keep, outs = extract_args(sized, capacities, download)
    for k in range(len(items)):
        cf[k].image.data = C.cast(None, capi.c_uint8_p)
    return cf, cr, keep, outs


def pyramid_cpu(items, download: bool = True, host_lib=None):
    """csrc/orb_pyramid.h on the host in one thread (osh_host_orb_pyramid_cpu of the test library): the per-item dicts of
    OrbMatcher.pyramid_build (token 0) and the wall time of the loops in ms."""
    host_lib = host_lib or capi.load_host_library()
    ms = C.c_double(0)
    cf, cr, _keep, outs = pyramid_args(items, download)
    rc = host_lib.osh_host_orb_pyramid_cpu(len(items), cf, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_orb_pyramid_cpu -> {rc}")
    return _pyramid_outputs(cr, outs), float(ms.value)


def compute_pyramid(image, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, host_lib=None) -> dict:
    """ORBextractor::ComputePyramid of the stand-in class on a uint8 image through osh_host_orbextractor_compute_pyramid: shapes,
    bordered (the whole images, 19 pixels around every level), built_token (after ComputePyramid, after the first
    ComputeKeyPointsOctTree), and the keypoints of ComputeKeyPointsOctTree right after it (level_count, xy, angle, response) and
    from a hand-set copy of the pyramid (hand_*)."""
    host_lib = host_lib or capi.load_host_library()
    cin = capi.HostExtractInput()
    _img = fill_host_extract_input(cin, image, nfeatures, scale_factor, nlevels, ini_th, min_th)
    arrays = lambda cap, pix: dict(
        level_rows=np.zeros(nlevels, np.int32), level_cols=np.zeros(nlevels, np.int32), bordered=np.zeros(max(pix, 1), np.uint8),
        pixels_needed=np.zeros(1, np.int32), built_token=np.zeros(2, np.uint64), level_count=np.zeros(nlevels, np.int32),
        xy=np.zeros((cap, 2), np.float32), angle=np.zeros(cap, np.float32), response=np.zeros(cap, np.float32),
        hand_level_count=np.zeros(nlevels, np.int32), hand_xy=np.zeros((cap, 2), np.float32), hand_angle=np.zeros(cap, np.float32),
        hand_response=np.zeros(cap, np.float32))
    _n, o = counted_call(host_lib.osh_host_orbextractor_compute_pyramid, "osh_host_orbextractor_compute_pyramid", cin, capi.HostPyramidOutput,
                         "pixel_capacity", arrays, lambda n, o: (n, int(o["pixels_needed"][0])))
    n1, n2 = int(o["level_count"].sum()), int(o["hand_level_count"].sum())
    out = dict(shapes=list(zip(o["level_rows"].tolist(), o["level_cols"].tolist())), built_token=[int(t) for t in o["built_token"]],
               level_count=o["level_count"], hand_level_count=o["hand_level_count"])
    for name in ("xy", "angle", "response"):
        out[name], out["hand_" + name] = o[name][:n1], o["hand_" + name][:n2]
    whole = cut_levels(o["bordered"], [(r + 38, c + 38) if r else (0, 0) for r, c in out["shapes"]])
    out["bordered"] = [w if r else None for w, (r, _) in zip(whole, out["shapes"])]
    return out


def ic_angle_args(items, borders=None):
    """The osh_ic_angle_frame / osh_ic_angle_result arrays for items dict(xy [n, 2], level [n], and pyramid (a list of levels) or
    token)."""
    n_items = len(items)
    cf = (capi.IcAngleFrame * max(n_items, 1))()
    cr = (capi.IcAngleResult * max(n_items, 1))()
    keep, outs = [], []
    for k, it in enumerate(items):
        a = dict(xy=np.ascontiguousarray(it["xy"], np.float32).reshape(-1, 2), level=np.ascontiguousarray(it["level"], np.int32))
        n = cf[k].n = a["level"].shape[0]
        cf[k].xy, cf[k].level = capi.ptr(a["xy"], capi.c_float_p), capi.ptr(a["level"], capi.c_int32_p)
        _fill_pyramid_or_token(cf[k], it, 0 if borders is None else int(borders[k]), a)
        o = dict(angle=np.zeros(n, np.float32), m10=np.zeros(n, np.int32), m01=np.zeros(n, np.int32))
        _wire_outputs(cr[k], o)
        keep.append(a)
        outs.append(o)
    return cf, cr, keep, outs


def fast_cpu(frames, host_lib=None, borders=None):
    """csrc/orb_fast.h on the host in one thread (osh_host_orb_fast_cpu of the test library): the per-frame dicts of
    OrbMatcher.fast_detect (token 0) and the wall time of the loops in ms."""
    host_lib = host_lib or capi.load_host_library()
    ms = C.c_double(0)
    cf, cr, _keep, outs = fast_args(frames, [(0, 0)] * len(frames), borders)
    if host_lib.osh_host_orb_fast_cpu(len(frames), cf, cr, None) != 0:
        raise RuntimeError("osh_host_orb_fast_cpu refused the frames")
    cf, cr, _keep, outs = fast_args(frames, [(cr[k].n_out, cr[k].n_cells) for k in range(len(frames))], borders)
    rc = host_lib.osh_host_orb_fast_cpu(len(frames), cf, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_orb_fast_cpu -> {rc}")
    return _fast_outputs(cr, outs), float(ms.value)


def ic_angle_cpu(items, host_lib=None, borders=None):
    """IC_Angle of csrc/orb_fast.h on the host in one thread (osh_host_orb_ic_angle_cpu); every item brings its pyramid."""
    host_lib = host_lib or capi.load_host_library()
    ms = C.c_double(0)
    cf, cr, _keep, outs = ic_angle_args(items, borders)
    rc = host_lib.osh_host_orb_ic_angle_cpu(len(items), cf, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_orb_ic_angle_cpu -> {rc}")
    return outs, float(ms.value)


_POINTER[np.dtype(np.int8)] = C.POINTER(C.c_int8)
_POINTER[np.dtype(np.uint16)] = C.POINTER(C.c_uint16)


def describe_args(items, borders=None, debug: bool = False):
    """The osh_describe_frame / osh_describe_result arrays for items dict(xy [n, 2], level [n], angle [n], pattern [512, 2], and
    pyramid (a list of levels) or token with shapes (the level shapes, needed only for `debug`), optionally blur_q8 [7])."""
    n_items = len(items)
    cf = (capi.DescribeFrame * max(n_items, 1))()
    cr = (capi.DescribeResult * max(n_items, 1))()
    keep, outs = [], []
    for k, it in enumerate(items):
        a = dict(xy=np.ascontiguousarray(it["xy"], np.float32).reshape(-1, 2), level=np.ascontiguousarray(it["level"], np.int32),
                 angle=np.ascontiguousarray(it["angle"], np.float32))
        n = cf[k].n = a["level"].shape[0]
        _wire_outputs(cf[k], a)
        if it.get("pattern") is not None:
            a["pattern"] = np.ascontiguousarray(it["pattern"], np.int8).reshape(-1)
            assert a["pattern"].shape[0] == 1024
            cf[k].pattern = capi.ptr(a["pattern"], _POINTER[a["pattern"].dtype])
        if it.get("blur_q8") is not None:
            a["blur_q8"] = np.ascontiguousarray(it["blur_q8"], np.uint16).reshape(-1)
            assert a["blur_q8"].shape[0] == 7
            cf[k].blur_q8 = capi.ptr(a["blur_q8"], _POINTER[a["blur_q8"].dtype])
        _fill_pyramid_or_token(cf[k], it, 0 if borders is None else int(borders[k]), a)
        if it.get("pyramid") is not None:
            shapes = [(0, 0) if p is None else tuple(p.shape) for p in it["pyramid"]]
        else:
            shapes = [tuple(s) for s in it.get("shapes", ())]
        o = dict(descriptors=np.zeros((n, 32), np.uint8))
        if debug:
            o.update(cos_sin=np.zeros((n, 2), np.float32), blurred=np.zeros(max(sum(r * c for r, c in shapes), 1), np.uint8))
        _wire_outputs(cr[k], o)
        o["shapes"] = shapes
        keep.append(a)
        outs.append(o)
    return cf, cr, keep, outs


def _describe_outputs(outs):
    """`blurred` cut into the levels of the item."""
    res = []
    for o in outs:
        d = {k: v for k, v in o.items() if k != "shapes"}
        if "blurred" in d:
            d["blurred"] = cut_levels(d["blurred"], o["shapes"], copy=False)
        res.append(d)
    return res


def describe_cpu(items, host_lib=None, borders=None, debug: bool = False):
    """csrc/orb_brief.h on the host in one thread (osh_host_orb_describe_cpu of the test library); every item brings its pyramid.
    Returns the per-item dicts of OrbMatcher.describe and the wall time of the loops in ms."""
    host_lib = host_lib or capi.load_host_library()
    ms = C.c_double(0)
    cf, cr, _keep, outs = describe_args(items, borders, debug)
    rc = host_lib.osh_host_orb_describe_cpu(len(items), cf, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_orb_describe_cpu -> {rc}")
    return _describe_outputs(outs), float(ms.value)


def brief_gaussian_q8(ksize: int = 7, sigma: float = 2.0, host_lib=None) -> np.ndarray:
    """brief_gaussian_q8 of csrc/orb_brief.h: the default blur weights for (7, 2)."""
    host_lib = host_lib or capi.load_host_library()
    out = np.zeros(int(ksize), np.uint16)
    if host_lib.osh_host_brief_gaussian_q8(int(ksize), float(sigma), capi.ptr(out, _POINTER[out.dtype])) != 0:
        raise RuntimeError("osh_host_brief_gaussian_q8 refused its arguments")
    return out


def brief_reach(pattern, host_lib=None) -> int:
    """brief_reach of csrc/orb_brief.h: ceil of the largest radius of a table [512, 2]."""
    host_lib = host_lib or capi.load_host_library()
    p = np.ascontiguousarray(pattern, np.int8).reshape(-1)
    assert p.shape[0] == 1024
    return int(host_lib.osh_host_brief_reach(capi.ptr(p, _POINTER[p.dtype])))


def standin_pattern(host_lib=None) -> np.ndarray:
    """The sampling table [512, 2] the stand-in ORBextractor constructor generates."""
    host_lib = host_lib or capi.load_host_library()
    p = np.zeros(1024, np.int8)
    if host_lib.osh_host_orbextractor_pattern(capi.ptr(p, _POINTER[p.dtype])) != 0:
        raise RuntimeError("osh_host_orbextractor_pattern failed")
    return p.reshape(512, 2)


def extract(image, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, lapping=(0, 0), host_lib=None) -> dict:
    """ORBextractor::operator() of the stand-in class on a uint8 image (None or an empty array: an empty image) through
    osh_host_orbextractor_extract: ret, desc_rows, the pyramid ComputePyramid built (a list of levels), the per-level keypoints of
    ComputeKeyPointsOctTree (level_count, level_xy, level_angle) and _keypoints (xy, angle, size, response, octave) with
    descriptors [n, 32]; call_ms is the wall time of the operator() call alone."""
    host_lib = host_lib or capi.load_host_library()
    cin = capi.HostExtractInput()
    _img = fill_host_extract_input(cin, image, nfeatures, scale_factor, nlevels, ini_th, min_th, lapping)
    arrays = lambda cap, pix: dict(
        level_rows=np.zeros(nlevels, np.int32), level_cols=np.zeros(nlevels, np.int32), pyramid=np.zeros(max(pix, 1), np.uint8),
        level_count=np.zeros(nlevels, np.int32), level_xy=np.zeros((cap, 2), np.float32), level_angle=np.zeros(cap, np.float32),
        xy=np.zeros((cap, 2), np.float32), angle=np.zeros(cap, np.float32), size=np.zeros(cap, np.float32),
        response=np.zeros(cap, np.float32), octave=np.zeros(cap, np.int32), descriptors=np.zeros((cap, 32), np.uint8),
        ret=np.zeros(1, np.int32), desc_rows=np.zeros(1, np.int32), pixels_needed=np.zeros(1, np.int32), call_ms=np.zeros(1, np.float64))
    n, o = counted_call(host_lib.osh_host_orbextractor_extract, "osh_host_orbextractor_extract", cin, capi.HostExtractOutput, "pixel_capacity", arrays,
                        lambda n, o: (max(n, int(o["level_count"].sum())), int(o["pixels_needed"][0])))
    nl = int(o["level_count"].sum())
    out = dict(ret=int(o["ret"][0]), desc_rows=int(o["desc_rows"][0]), call_ms=float(o["call_ms"][0]), n=n, level_count=o["level_count"], level_xy=o["level_xy"][:nl],
               level_angle=o["level_angle"][:nl])
    for name in ("xy", "angle", "size", "response", "octave", "descriptors"):
        out[name] = o[name][:n]
    out["pyramid"] = cut_levels(o["pyramid"], zip(o["level_rows"].tolist(), o["level_cols"].tolist()))
    return out


def bow_tree(tree):
    """capi.BowTree of a synth_bow.BowTree and the arrays its pointers refer to."""
    keep = (np.ascontiguousarray(tree.parent, np.int32), np.ascontiguousarray(tree.is_leaf, np.uint8),
            np.ascontiguousarray(tree.desc, np.uint8), np.ascontiguousarray(tree.weight, np.float64))
    t = capi.BowTree()
    t.k, t.L, t.weighting, t.scoring, t.n = int(tree.k), int(tree.L), int(tree.weighting), int(tree.scoring), keep[0].shape[0]
    t.parent, t.is_leaf = capi.ptr(keep[0], capi.c_int32_p), capi.ptr(keep[1], capi.c_uint8_p)
    t.desc, t.weight = capi.ptr(keep[2], capi.c_uint8_p), capi.ptr(keep[3], capi.c_double_p)
    return t, keep


def bow_outputs(n: int, stages: bool = True) -> dict:
    """The arrays of an osh_bow_result for a frame of n features."""
    o = dict(n_words=np.zeros(1, np.int32), word_id=np.zeros(n, np.int32), word_value=np.zeros(n, np.float64),
             n_nodes=np.zeros(1, np.int32), node_id=np.zeros(n, np.int32), node_start=np.zeros(n + 1, np.int32),
             node_feat=np.zeros(n, np.int32))
    if stages:
        o.update(feat_word=np.zeros(n, np.int32), feat_node=np.zeros(n, np.int32), feat_dist=np.zeros(n, np.int32))
    return o


def bow_trim(o: dict) -> dict:
    """The outputs cut to the entries the call filled: n_words words, n_nodes nodes and their features."""
    nw, nn = int(o["n_words"][0]), int(o["n_nodes"][0])
    t = dict(o, word_id=o["word_id"][:nw], word_value=o["word_value"][:nw], node_id=o["node_id"][:nn], node_start=o["node_start"][:nn + 1])
    t["node_feat"] = o["node_feat"][:int(t["node_start"][nn])]
    del t["n_words"], t["n_nodes"]
    return t


def bow_args(frames, stages: bool = False):
    """The osh_bow_frame / osh_bow_result arrays of OrbMatcher.bow_transform for repeated calls: (frames, results, the arrays that
    keep their pointers alive, the per-frame dicts of output arrays)."""
    n_frames = len(frames)
    cf = (capi.BowFrame * max(n_frames, 1))()
    cr = (capi.BowResult * max(n_frames, 1))()
    keep, outs = [], []
    for k, fr in enumerate(frames):
        d = np.ascontiguousarray(fr, dtype=np.uint8).reshape(-1, 32)
        cf[k].n, cf[k].desc = d.shape[0], capi.ptr(d, capi.c_uint8_p)
        o = bow_outputs(d.shape[0], stages)
        _wire_outputs(cr[k], o)
        keep.append(d)
        outs.append(o)
    return cf, cr, keep, outs


def bow_db_args(queries, capacity: int):
    """The osh_bow_db_query / osh_bow_db_result arrays of OrbMatcher.bow_db_query for repeated calls: (queries, results, the arrays
    that keep their pointers alive, the per-query dicts of output arrays of `capacity` entries)."""
    n = len(queries)
    cq = (capi.BowDbQuery * max(n, 1))()
    cr = (capi.BowDbResult * max(n, 1))()
    keep, outs = [], []
    for k, q in enumerate(queries):
        w, v = np.ascontiguousarray(q[0], np.int32), np.ascontiguousarray(q[1], np.float64)
        ex = np.ascontiguousarray(q[2] if len(q) > 2 else [], np.uint64)
        assert w.shape == v.shape and w.ndim == 1
        cq[k].n, cq[k].word_id, cq[k].value = w.shape[0], capi.ptr(w, capi.c_int32_p), capi.ptr(v, capi.c_double_p)
        cq[k].n_excluded, cq[k].excluded = ex.shape[0], capi.ptr(ex, C.POINTER(C.c_uint64))
        o = dict(max_common=np.zeros(1, np.int32), min_common=np.zeros(1, np.int32), n_rows=np.zeros(1, np.int32),
                 handle=np.zeros(capacity, np.uint64), common=np.zeros(capacity, np.int32), first_word=np.zeros(capacity, np.int32),
                 scored=np.zeros(capacity, np.uint8), score=np.zeros(capacity, np.float64))
        cr[k].capacity = capacity
        _wire_outputs(cr[k], o)
        keep.append((w, v, ex))
        outs.append(o)
    return cq, cr, keep, outs


def bow_db_trim(o: dict) -> dict:
    """The outputs of a query cut to its listed rows; max_common and min_common as ints."""
    n = int(o["n_rows"][0])
    t = {k: o[k][:n] for k in ("handle", "common", "first_word", "scored", "score")}
    t.update(max_common=int(o["max_common"][0]), min_common=int(o["min_common"][0]))
    return t


def fisheye_stereo_args(frames, stages: bool = False):
    """The osh_fisheye_stereo_frame / osh_fisheye_stereo_result arrays of OrbMatcher.fisheye_stereo_match for repeated calls:
    (frames, results, the arrays that keep their pointers alive, the per-frame dicts of output arrays)."""
    n_frames = len(frames)
    cf = (capi.FisheyeStereoFrame * max(n_frames, 1))()
    cr = (capi.FisheyeStereoResult * max(n_frames, 1))()
    keep, outs = [], []
    for k, fr in enumerate(frames):
        a = fill_fisheye_frame(cf[k], fr)
        nl, nr = cf[k].n_left, cf[k].n_right
        o = dict(left_to_right=np.zeros(nl, np.int32), right_to_left=np.zeros(nr, np.int32), depth=np.zeros(nl, np.float32),
                 p3d=np.zeros((nl, 3), np.float32))
        if stages:
            o.update(best_right=np.zeros(nl, np.int32), best_dist=np.zeros(nl, np.int32), second_dist=np.zeros(nl, np.int32),
                     cos_parallax=np.zeros(nl, np.float32), stage=np.zeros(nl, np.uint8))
        _wire_outputs(cr[k], o)
        keep.append(a)
        outs.append(o)
    return cf, cr, keep, outs


def fill_fisheye_frame(f, fr, a=None):
    """The fields capi.FisheyeStereoFrame and capi.HostFisheyeInput share, from a synth_fisheye.FisheyeFrame; a: its contiguous
    arrays (the six of the keypoints and sig) if the caller made them already.  Returns the arrays the pointers refer to."""
    a = _fill_keypoints(f, fr, a)
    a.setdefault("sig", np.ascontiguousarray(fr.level_sigma2, np.float32))
    f.mono_left, f.mono_right = int(fr.mono_left), int(fr.mono_right)
    f.n_levels, f.level_sigma2 = a["sig"].shape[0], capi.ptr(a["sig"], capi.c_float_p)
    f.cam1[:] = [float(x) for x in np.asarray(fr.cam1, np.float32)]
    f.cam2[:] = [float(x) for x in np.asarray(fr.cam2, np.float32)]
    f.precision1, f.precision2 = float(fr.precision1), float(fr.precision2)
    f.Rlr[:] = [float(x) for x in np.asarray(fr.Rlr, np.float32).reshape(9)]
    f.tlr[:] = [float(x) for x in np.asarray(fr.tlr, np.float32)]
    return a


def _fill_newpoint_pose(p, pose):
    p.Rcw[:] = [float(x) for x in np.asarray(pose.Rcw, np.float32).reshape(9)]
    p.tcw[:] = [float(x) for x in np.asarray(pose.tcw, np.float32)]
    p.Rwc[:] = [float(x) for x in np.asarray(pose.Rwc, np.float32).reshape(9)]
    p.Ow[:] = [float(x) for x in np.asarray(pose.Ow, np.float32)]


def _fill_newpoint_camera(c, cam):
    c.type, c.precision = int(cam.type), float(cam.precision)
    c.params[:] = [float(x) for x in np.asarray(cam.params, np.float32)]


def fill_newpoint_keyframe(k, kf):
    """capi.NewPointKeyFrame from a synth_newpoints.KeyFrame; returns the arrays its pointers refer to."""
    _fill_newpoint_pose(k.pose, kf.pose)
    _fill_newpoint_camera(k.camera, kf.camera)
    k.has_camera2 = int(kf.camera2 is not None)
    if kf.camera2 is not None:
        _fill_newpoint_pose(k.right_pose, kf.right_pose)
        _fill_newpoint_camera(k.camera2, kf.camera2)
    for name in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf", "mb"):
        setattr(k, name, float(getattr(kf, name)))
    keep = (np.ascontiguousarray(kf.level_sigma2, np.float32), np.ascontiguousarray(kf.scale_factors, np.float32))
    k.n_left, k.n_keys, k.n_levels = int(kf.n_left), int(kf.n_keys), keep[0].shape[0]
    k.level_sigma2, k.scale_factors = capi.ptr(keep[0], capi.c_float_p), capi.ptr(keep[1], capi.c_float_p)
    return keep


_NEWPOINT_ARRAYS = (("idx1", np.int32), ("idx2", np.int32), ("pt1", np.float32), ("pt2", np.float32), ("octave1", np.int32),
                    ("octave2", np.int32), ("u_right1", np.float32), ("u_right2", np.float32), ("depth1", np.float32), ("depth2", np.float32))


def newpoint_args(segments):
    """The osh_newpoint_segment / osh_newpoint_result arrays of OrbMatcher.triangulate_new_points for repeated calls: (segments,
    results, the arrays that keep their pointers alive, the per-segment dicts of output arrays)."""
    n_seg = len(segments)
    cs = (capi.NewPointSegment * max(n_seg, 1))()
    cr = (capi.NewPointResult * max(n_seg, 1))()
    keep, outs = [], []
    for k, sg in enumerate(segments):
        c = cs[k]
        a = {"kf1": fill_newpoint_keyframe(c.kf1, sg.kf1), "kf2": fill_newpoint_keyframe(c.kf2, sg.kf2)}
        c.ratio_factor, c.inertial, c.far_points, c.th_far_points = float(sg.ratio_factor), int(sg.inertial), int(sg.far_points), float(sg.th_far_points)
        n = c.n_matches = int(np.asarray(sg.idx1).shape[0])
        for name, dt in _NEWPOINT_ARRAYS:
            a[name] = np.ascontiguousarray(getattr(sg, name), dt)
            setattr(c, name, capi.ptr(a[name], _POINTER[np.dtype(dt)]))
        o = dict(stage=np.zeros(n, np.uint8), source=np.zeros(n, np.uint8), cos_parallax=np.zeros(n, np.float32), x3d=np.zeros((n, 3), np.float32))
        _wire_outputs(cr[k], o)
        keep.append(a)
        outs.append(o)
    return cs, cr, keep, outs


def newpoint_cpu(segments, host_lib=None):
    """csrc/newpoint_triangulate.h on the host in one thread (osh_host_newpoint_triangulate_cpu of the test library): the per-segment
    output dicts of triangulate_new_points and the wall time of the loops in ms."""
    host_lib = host_lib or capi.load_host_library()
    cs, cr, _keep, outs = newpoint_args(segments)
    ms = C.c_double(0)
    rc = host_lib.osh_host_newpoint_triangulate_cpu(len(segments), cs, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_newpoint_triangulate_cpu -> {rc}")
    return outs, float(ms.value)


def mask_bits(mask, n: int) -> np.ndarray:
    """The flags [.., n] of inlier mask words [.., words] (bit i % 32 of word i / 32 is correspondence i)."""
    m = np.ascontiguousarray(mask, np.uint32)
    bits = np.unpackbits(m.view(np.uint8).reshape(m.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)


mlpnp_mask_bits = mask_bits   # the name callers written against the MLPnP entry use


def _ransac_outputs(res, a, o, fill, keep, outs):
    """The tail of two_view_args, mlpnp_args and sim3_ransac_args for one problem: the output arrays o pre-filled with the byte
    `fill` (None: left as they are) and wired into the result struct, o and the input arrays a appended to outs and keep."""
    if fill is not None:
        for v in o.values():
            v.view(np.uint8)[...] = fill
    _wire_outputs(res, o)
    keep.append(a)
    outs.append(o)


def _ransac_cpu(symbol, args, problems, debug, host_lib):
    """The host build of a RANSAC entry in one thread (`symbol` of the test library) on what `args` builds: the per-problem output
    dicts and the wall time in ms."""
    host_lib = host_lib or capi.load_host_library()
    cp, cr, _keep, outs = args(problems, debug)
    ms = C.c_double(0)
    rc = getattr(host_lib, symbol)(len(problems), cp, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"{symbol} -> {rc}")
    return outs, float(ms.value)


def _ransac_check_inliers(call, args, problem, transforms, dtype, width):
    """CheckInliers of the transforms [k, width] against one problem through call(problem, k, transforms, count, mask): its return
    code, count [k], mask [k, words]."""
    cp, _cr, _keep, _outs = args([problem])
    T = np.ascontiguousarray(transforms, dtype).reshape(-1, width)
    count = np.zeros(T.shape[0], np.int32)
    mask = np.zeros((T.shape[0], capi.ransac_mask_words(problem.n)), np.uint32)
    rc = call(cp, T.shape[0], capi.ptr(T, _POINTER[np.dtype(dtype)]), capi.ptr(count, capi.c_int32_p), capi.ptr(mask, capi.c_uint32_p))
    return rc, count, mask


def _ransac_check_inliers_cpu(symbol, args, problem, transforms, dtype, width, host_lib):
    """The same on the host (`symbol` of the test library): count [k], mask [k, words]."""
    rc, count, mask = _ransac_check_inliers(getattr(host_lib or capi.load_host_library(), symbol), args, problem, transforms, dtype, width)
    if rc != 0:
        raise RuntimeError(f"{symbol} -> {rc}")
    return count, mask


_TWOVIEW_ARRAYS = (("idx1", np.int32), ("idx2", np.int32), ("pt1", np.float32), ("pt2", np.float32), ("pn1", np.float32),
                   ("pn2", np.float32), ("sets", np.int32))


def two_view_args(problems, debug: bool = False, fill=None):
    """The osh_two_view_problem / osh_two_view_result arrays of OrbMatcher.two_view_reconstruct for repeated calls: (problems,
    results, the arrays that keep their pointers alive, the per-problem dicts of output arrays).  fill: a byte the output arrays
    are pre-filled with (None: zeros)."""
    n_p = len(problems)
    cp = (capi.TwoViewProblem * max(n_p, 1))()
    cr = (capi.TwoViewResult * max(n_p, 1))()
    keep, outs = [], []
    for k, pb in enumerate(problems):
        c = cp[k]
        c.K[:] = [float(x) for x in np.asarray(pb.K, np.float32).reshape(9)]
        c.T1[:] = [float(x) for x in np.asarray(pb.T1, np.float32).reshape(9)]
        c.T2[:] = [float(x) for x in np.asarray(pb.T2, np.float32).reshape(9)]
        a = {name: np.ascontiguousarray(getattr(pb, name), dt) for name, dt in _TWOVIEW_ARRAYS}
        n, it = a["idx1"].shape[0], a["sets"].reshape(-1, 8).shape[0]
        c.sigma, c.n_iterations, c.n_matches, c.n_keys1, c.n_keys2 = float(pb.sigma), it, n, int(pb.n_keys1), int(pb.n_keys2)
        for name, dt in _TWOVIEW_ARRAYS:
            setattr(c, name, capi.ptr(a[name], _POINTER[np.dtype(dt)]))
        f32, i32 = np.float32, np.int32
        o = dict(status=np.zeros(1, i32), T21=np.zeros(12, f32), sh=np.zeros(1, f32), sf=np.zeros(1, f32), H21=np.zeros((3, 3), f32),
                 F21=np.zeros((3, 3), f32), best_h=np.zeros(1, i32), best_f=np.zeros(1, i32), info=np.zeros(4, i32),
                 inlier=np.zeros(n, np.uint8), x3d=np.zeros((n, 3), f32), triangulated=np.zeros(n, np.uint8), n_good=np.zeros(8, i32),
                 parallax=np.zeros(8, f32))
        if debug:
            o.update(debug_model_n=np.zeros((2, it, 3, 3), f32), debug_model=np.zeros((2, it, 3, 3), f32), debug_score=np.zeros((2, it), f32),
                     debug_R=np.zeros((8, 3, 3), f32), debug_t=np.zeros((8, 3), f32))
        _ransac_outputs(cr[k], a, o, fill, keep, outs)
    return cp, cr, keep, outs


def two_view_cpu(problems, debug: bool = False, host_lib=None):
    """csrc/two_view.h on the host in one thread (osh_host_two_view_cpu of the test library): the per-problem output dicts of
    two_view_reconstruct and the wall time in ms."""
    return _ransac_cpu("osh_host_two_view_cpu", two_view_args, problems, debug, host_lib)


_MLPNP_ARRAYS = (("bearing", np.float64), ("p3d", np.float64), ("p2d", np.float32), ("max_error", np.float32), ("sets", np.int32))


def mlpnp_args(problems, debug: bool = False, fill=None):
    """The osh_mlpnp_problem / osh_mlpnp_result arrays of OrbMatcher.mlpnp_solve for repeated calls: (problems, results, the arrays
    that keep their pointers alive, the per-problem dicts of output arrays).  fill: a byte the output arrays are pre-filled with
    (None: zeros)."""
    n_p = len(problems)
    cp = (capi.MlpnpProblem * max(n_p, 1))()
    cr = (capi.MlpnpResult * max(n_p, 1))()
    keep, outs = [], []
    for k, pb in enumerate(problems):
        c = cp[k]
        a = {name: np.ascontiguousarray(getattr(pb, name), dt) for name, dt in _MLPNP_ARRAYS}
        n, it = a["p3d"].reshape(-1, 3).shape[0], a["sets"].reshape(-1, 6).shape[0]
        c.camera_type = int(pb.camera_type)
        c.camera[:] = [float(x) for x in np.asarray(pb.camera, np.float32).reshape(8)]
        c.n, c.n_iterations = n, it
        c.min_inliers, c.best_inliers_in, c.best_refine_ok_in = int(pb.min_inliers), int(pb.best_inliers_in), int(pb.best_refine_ok_in)
        for name, dt in _MLPNP_ARRAYS:
            setattr(c, name, capi.ptr(a[name], _POINTER[np.dtype(dt)]))
        i32, f64, words = np.int32, np.float64, capi.ransac_mask_words(n)
        o = dict(first_hit=np.zeros(1, i32), hit_record=np.zeros(1, i32), hit_pose=np.zeros(12, f64), hit_count=np.zeros(1, i32),
                 hit_mask=np.zeros(words, np.uint32), best_iteration=np.zeros(1, i32), best_count=np.zeros(1, i32),
                 best_mask=np.zeros(words, np.uint32), best_pose=np.zeros(12, f64), best_refine_ok=np.zeros(1, i32),
                 n_records=np.zeros(1, i32), debug_count=np.zeros(it, i32), debug_record=np.zeros(it, i32),
                 debug_record_count=np.zeros(it, i32))
        if debug:
            o.update(debug_pose=np.zeros((it, 12), f64), debug_record_pose=np.zeros((it, 12), f64))
        _ransac_outputs(cr[k], a, o, fill, keep, outs)
    return cp, cr, keep, outs


def mlpnp_cpu(problems, debug: bool = False, host_lib=None):
    """csrc/mlpnp.h on the host in one thread (osh_host_mlpnp_cpu of the test library): the per-problem output dicts of mlpnp_solve
    and the wall time in ms."""
    return _ransac_cpu("osh_host_mlpnp_cpu", mlpnp_args, problems, debug, host_lib)


def mlpnp_check_inliers_cpu(problem, poses, host_lib=None):
    """CheckInliers of csrc/mlpnp.h on the host (osh_host_mlpnp_check_inliers): count [k], mask [k, words]."""
    return _ransac_check_inliers_cpu("osh_host_mlpnp_check_inliers", mlpnp_args, problem, poses, np.float64, 12, host_lib)


def mlpnp_stage(name: str, *args, host_lib=None):
    """The stages of csrc/mlpnp.h on the host (osh_host_mlpnp_* of the test library).  "nullspace": f [3] -> N [3, 2].  "rank": S [3, 3]
    -> rank.  "null_vector": M [c, c] -> h [c].  "compute_pose": bearing, p3d [n, 3] -> pose [12], info [3].  "gauss_newton": bearing,
    p3d, x [6], max_iterations -> x [6], info [2].  "replay": count, min_inliers, best_in, ok_in, record_count -> record, out [7].  "ransac_parameters": N, probability, minInliers,
    maxIterations, minSet, epsilon -> (mRansacMinInliers, mRansacMaxIts)."""
    lib = host_lib or capi.load_host_library()
    d = lambda a: np.ascontiguousarray(a, np.float64)
    dp = lambda a: capi.ptr(a, capi.c_double_p)
    ip = lambda a: capi.ptr(a, capi.c_int32_p)
    if name == "nullspace":
        f, N = d(args[0]), np.zeros((3, 2))
        rc = lib.osh_host_mlpnp_nullspace(dp(f), dp(N))
        out = N
    elif name == "rank":
        S = d(args[0])
        return int(lib.osh_host_mlpnp_rank(dp(S)))
    elif name == "null_vector":
        M = d(args[0])
        h = np.zeros(M.shape[0])
        rc = lib.osh_host_mlpnp_null_vector(dp(M), M.shape[0], dp(h))
        out = h
    elif name == "compute_pose":
        f, p, pose, info = d(args[0]), d(args[1]), np.zeros(12), np.zeros(3, np.int32)
        rc = lib.osh_host_mlpnp_compute_pose(f.shape[0], dp(f), dp(p), dp(pose), ip(info))
        out = (pose, info)
    elif name == "gauss_newton":
        f, p, x, info = d(args[0]), d(args[1]), d(args[2]).copy(), np.zeros(2, np.int32)
        rc = lib.osh_host_mlpnp_gauss_newton(f.shape[0], dp(f), dp(p), dp(x), int(args[3]), ip(info))
        out = (x, info)
    elif name == "ransac_parameters":
        res = np.zeros(2, np.int32)
        rc = lib.osh_host_mlpnp_ransac_parameters(int(args[0]), float(args[1]), int(args[2]), int(args[3]), int(args[4]), float(args[5]), ip(res))
        out = (int(res[0]), int(res[1]))
    elif name == "replay":
        count, rcount = np.ascontiguousarray(args[0], np.int32), np.ascontiguousarray(args[4], np.int32)
        record, res = np.full(max(count.shape[0], 1), -1, np.int32), np.zeros(7, np.int32)
        rc = lib.osh_host_mlpnp_replay(count.shape[0], ip(count), int(args[1]), int(args[2]), int(args[3]), ip(rcount), ip(record), ip(res))
        out = (record[:int(res[6])], res)
    else:
        raise ValueError(name)
    if rc != 0:
        raise RuntimeError(f"osh_host_mlpnp_{name} -> {rc}")
    return out


_SIM3R_ARRAYS = (("x3dc1", np.float32), ("x3dc2", np.float32), ("p1im1", np.float32), ("p2im2", np.float32), ("max_error1", np.float32),
                 ("max_error2", np.float32), ("sets", np.int32))


def sim3_ransac_args(problems, debug: bool = False, fill=None):
    """The osh_sim3r_problem / osh_sim3r_result arrays of OrbMatcher.sim3_ransac for repeated calls: (problems, results, the arrays
    that keep their pointers alive, the per-problem dicts of output arrays).  fill: a byte the output arrays are pre-filled with
    (None: zeros)."""
    n_p = len(problems)
    cp = (capi.Sim3rProblem * max(n_p, 1))()
    cr = (capi.Sim3rResult * max(n_p, 1))()
    keep, outs = [], []
    for k, pb in enumerate(problems):
        c = cp[k]
        a = {name: np.ascontiguousarray(getattr(pb, name), dt) for name, dt in _SIM3R_ARRAYS}
        n, it = a["x3dc1"].reshape(-1, 3).shape[0], a["sets"].reshape(-1, 3).shape[0]
        c.camera_type1, c.camera_type2 = int(pb.camera_type1), int(pb.camera_type2)
        c.camera1[:] = [float(x) for x in np.asarray(pb.camera1, np.float32).reshape(8)]
        c.camera2[:] = [float(x) for x in np.asarray(pb.camera2, np.float32).reshape(8)]
        c.fix_scale, c.n, c.n_iterations = int(pb.fix_scale), n, it
        c.min_inliers, c.best_inliers_in = int(pb.min_inliers), int(pb.best_inliers_in)
        for name, dt in _SIM3R_ARRAYS:
            setattr(c, name, capi.ptr(a[name], _POINTER[np.dtype(dt)]))
        i32, f32, words = np.int32, np.float32, capi.ransac_mask_words(n)
        o = dict(first_hit=np.zeros(1, i32), n_records=np.zeros(1, i32), record=np.zeros(it, i32), record_count=np.zeros(it, i32),
                 record_T=np.zeros((it, 13), f32), record_mask=np.zeros((it, words), np.uint32), best_iteration=np.zeros(1, i32),
                 best_count=np.zeros(1, i32), debug_count=np.zeros(it, i32))
        if debug:
            o.update(debug_T=np.zeros((it, 13), f32))
        _ransac_outputs(cr[k], a, o, fill, keep, outs)
    return cp, cr, keep, outs


def sim3_ransac_cpu(problems, debug: bool = False, host_lib=None):
    """csrc/sim3_ransac.h on the host in one thread (osh_host_sim3r_cpu of the test library): the per-problem output dicts of
    sim3_ransac and the wall time in ms."""
    return _ransac_cpu("osh_host_sim3r_cpu", sim3_ransac_args, problems, debug, host_lib)


def sim3_ransac_check_inliers_cpu(problem, T12s, host_lib=None):
    """CheckInliers of csrc/sim3_ransac.h on the host (osh_host_sim3r_check_inliers): count [k], mask [k, words]."""
    return _ransac_check_inliers_cpu("osh_host_sim3r_check_inliers", sim3_ransac_args, problem, T12s, np.float32, 13, host_lib)


def sim3_ransac_stage(name: str, *args, host_lib=None):
    """The stages of csrc/sim3_ransac.h on the host (osh_host_sim3r_* of the test library).  "compute_sim3": P1, P2 [3, 3] (the set's
    members in camera 1 and camera 2), fix_scale -> T [13].  "scan": count, min_inliers, best_in -> record, out [4] (first_hit,
    n_records, best_iteration, best_count).  "max_iterations": N, probability, minInliers, maxIterations -> mRansacMaxIts."""
    lib = host_lib or capi.load_host_library()
    if name == "compute_sim3":
        P1, P2, T = np.ascontiguousarray(args[0], np.float32), np.ascontiguousarray(args[1], np.float32), np.zeros(13, np.float32)
        rc = lib.osh_host_sim3r_compute_sim3(capi.ptr(P1, capi.c_float_p), capi.ptr(P2, capi.c_float_p), int(args[2]), capi.ptr(T, capi.c_float_p))
        out = T
    elif name == "scan":
        count = np.ascontiguousarray(args[0], np.int32)
        record, res = np.full(max(count.shape[0], 1), -1, np.int32), np.zeros(4, np.int32)
        rc = lib.osh_host_sim3r_scan(count.shape[0], capi.ptr(count, capi.c_int32_p), int(args[1]), int(args[2]), capi.ptr(record, capi.c_int32_p),
                                     capi.ptr(res, capi.c_int32_p))
        out = (record[:int(res[1])], res)
    elif name == "max_iterations":
        return int(lib.osh_host_sim3r_max_iterations(int(args[0]), float(args[1]), int(args[2]), int(args[3])))
    else:
        raise ValueError(name)
    if rc != 0:
        raise RuntimeError(f"osh_host_sim3r_{name} -> {rc}")
    return out


_MAPPOINT_ARRAYS = (("entry_off", np.int32), ("desc", np.uint8), ("centre", np.int32), ("use_desc", np.uint8), ("centres", np.float32),
                    ("pos", np.float32), ("ref_centre", np.int32), ("level_scale", np.float32), ("top_scale", np.float32))
MAPPOINT_OUTPUTS = ("best_entry", "best_median", "normal", "min_distance", "max_distance")


def mappoint_outputs(n: int, want=None, fill=None) -> dict:
    """The output arrays of one batch of n points; fill = (int32 value, float32 value) presets them (default zeros)."""
    ifill, ffill = (0, 0.0) if fill is None else fill
    o = dict(best_entry=np.full(n, ifill, np.int32), best_median=np.full(n, ifill, np.int32), normal=np.full((n, 3), ffill, np.float32),
             min_distance=np.full(n, ffill, np.float32), max_distance=np.full(n, ffill, np.float32))
    return {k: v for k, v in o.items() if want is None or k in want}


def mappoint_args(batches, want=None, fill=None):
    """The osh_mappoint_batch / osh_mappoint_result arrays of OrbMatcher.refresh_map_points for repeated calls: (batches, results,
    the arrays that keep their pointers alive, the per-batch dicts of output arrays).  Outputs not in `want` stay NULL."""
    n_b = len(batches)
    cb = (capi.MapPointBatch * max(n_b, 1))()
    cr = (capi.MapPointResult * max(n_b, 1))()
    keep, outs = [], []
    for k, b in enumerate(batches):
        c = cb[k]
        a = {}
        for name, dt in _MAPPOINT_ARRAYS:
            a[name] = np.ascontiguousarray(getattr(b, name), dt)
            setattr(c, name, capi.ptr(a[name], _POINTER[np.dtype(dt)]))
        c.n_points = int(a["entry_off"].shape[0]) - 1
        c.n_centres = int(a["centres"].reshape(-1, 3).shape[0])
        o = mappoint_outputs(c.n_points, want, fill)
        _wire_outputs(cr[k], o)
        keep.append(a)
        outs.append(o)
    return cb, cr, keep, outs


def mappoint_cpu(batches, host_lib=None):
    """csrc/mappoint_refresh.h on the host in one thread (osh_host_mappoint_refresh_cpu of the test library): the per-batch output
    dicts of refresh_map_points and the wall time of the loops in ms."""
    host_lib = host_lib or capi.load_host_library()
    cb, cr, _keep, outs = mappoint_args(batches)
    ms = C.c_double(0)
    rc = host_lib.osh_host_mappoint_refresh_cpu(len(batches), cb, cr, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_mappoint_refresh_cpu -> {rc}")
    return outs, float(ms.value)


_KFCULL_ARRAYS = (("cand_slot_off", np.int32), ("slot_point", np.int32), ("slot_level", np.int32), ("point_n_obs", np.int32),
                  ("point_bad", np.uint8), ("point_obs_off", np.int32), ("obs_kf", np.int32), ("obs_level", np.int32), ("obs_weight", np.int32))


def kfcull_problem(problem):
    """The osh_kfcull_problem of a synth_keyframe_cull.CullProblem and the arrays that keep its pointers alive."""
    cp = capi.KfCullProblem()
    cp.n_keyframes, cp.n_candidates, cp.redundant_th = int(problem.n_keyframes), int(problem.n_candidates), float(problem.redundant_th)
    cp.n_points = int(problem.n_points)
    keep = {}
    for name, dt in _KFCULL_ARRAYS:
        keep[name] = np.ascontiguousarray(getattr(problem, name), dt)
        setattr(cp, name, capi.ptr(keep[name], capi.c_int32_p if dt is np.int32 else capi.c_uint8_p))
    return cp, keep


def kfcull_result(n: int, fill: int = 0):
    out = {"n_mps": np.full(n, fill, np.int32), "n_redundant": np.full(n, fill, np.int32), "redundant": np.full(n, fill, np.uint8)}
    cr = capi.KfCullResult(capi.ptr(out["n_mps"], capi.c_int32_p), capi.ptr(out["n_redundant"], capi.c_int32_p), capi.ptr(out["redundant"], capi.c_uint8_p))
    return out, cr


def kfcull_cpu(problem, removed=(), first_candidate: int = 0, host_lib=None):
    """csrc/keyframe_cull.h on the host in one thread (osh_host_keyframe_cull_cpu of the test library): the dict of
    keyframe_cull_count and the wall time of the counting loop in ms."""
    host_lib = host_lib or capi.load_host_library()
    cp, _keep = kfcull_problem(problem)
    out, cr = kfcull_result(max(0, int(problem.n_candidates) - first_candidate))
    rm = np.ascontiguousarray(removed, np.int32).reshape(-1)
    ms = C.c_double(0)
    rc = host_lib.osh_host_keyframe_cull_cpu(C.byref(cp), len(rm), capi.ptr(rm, capi.c_int32_p), int(first_candidate), C.byref(cr), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_keyframe_cull_cpu -> {rc}")
    return out, float(ms.value)


def kb8_rig(cam1, cam2, precision1, precision2, R12, t12) -> "capi.Kb8Rig":
    g = capi.Kb8Rig()
    g.cam1[:] = [float(x) for x in np.asarray(cam1, np.float32)]
    g.cam2[:] = [float(x) for x in np.asarray(cam2, np.float32)]
    g.precision1, g.precision2 = float(precision1), float(precision2)
    g.R12[:] = [float(x) for x in np.asarray(R12, np.float32).reshape(9)]
    g.t12[:] = [float(x) for x in np.asarray(t12, np.float32)]
    return g


def kb8_pairs(xy1, xy2, sigma1, sigma2):
    """The four input arrays of osh_kb8_triangulate, contiguous float32."""
    f32 = lambda x, shape: np.ascontiguousarray(np.asarray(x, np.float32).reshape(shape))
    return f32(xy1, (-1, 2)), f32(xy2, (-1, 2)), f32(sigma1, (-1,)), f32(sigma2, (-1,))


def accept_local_points(res: dict, pair_index: int, nn_ratio: float = 0.8, th_high: int = 100) -> np.ndarray:
    """Acceptance rule of SearchByProjection(Frame&, vector<MapPoint*>&), src/ORBmatcher.cc:123-139,
    applied independently per query (no occupancy): bool mask of accepted queries."""
    bd = res["best_dist"][pair_index]
    sd = res["second_dist"][pair_index]
    bl, sl = res["best_level"][pair_index], res["second_level"][pair_index]
    ratio_fail = (bl == sl) & (bd.astype(np.float32) > np.float32(nn_ratio) * sd.astype(np.float32))
    return (bd <= th_high) & ~ratio_fail


def replay_local_points(res: dict, pair_index: int, rescan, nn_ratio: float = 0.8, th_high: int = 100,
                        occupied: np.ndarray | None = None, n_train: int | None = None):
    """Host side of SearchByProjection(Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:43-141) on top of the
    device search (SURVEY.md 8a "bit-exactness rule"): walk the queries in order; a query whose best or
    second-best slot was claimed by an earlier accepted query is re-scanned by `rescan(q, occupied)`
    -> (best_idx, best_dist, second_dist, best_level, second_level); occupancy only ever removes candidates,
    so every other query keeps its device result.  Returns (nmatches, assignment[n_train], n_rescans)."""
    bi, bd, sd = res["best_idx"][pair_index], res["best_dist"][pair_index], res["second_dist"][pair_index]
    bl, sl, si = res["best_level"][pair_index], res["second_level"][pair_index], res["second_idx"][pair_index]
    n_train = int(n_train if n_train is not None else max(int(bi.max()), int(si.max())) + 1)
    occ = np.zeros(n_train, dtype=np.uint8) if occupied is None else occupied
    pre_occupied = bool(occ.any())
    assign = -np.ones(n_train, dtype=np.int32)
    nmatches = rescans = 0
    ratio = np.float32(nn_ratio)
    for q in range(bi.shape[0]):
        b, d1, d2, l1, l2 = int(bi[q]), int(bd[q]), int(sd[q]), int(bl[q]), int(sl[q])
        if pre_occupied or (b >= 0 and occ[b]) or (si[q] >= 0 and occ[si[q]]):
            b, d1, d2, l1, l2 = rescan(q, occ)
            rescans += 1
        if b < 0 or d1 > th_high:
            continue
        if l1 == l2 and np.float32(d1) > ratio * np.float32(d2):
            continue
        assign[b] = q
        occ[b] = 1
        nmatches += 1
    return nmatches, assign, rescans


def frustum_frame(Rcw, tcw, fx, fy, cx, cy, bf, bounds, log_scale_factor, n_scale_levels, viewing_cos_limit=0.5, kb8=None):
    """osh_frustum_frame from a float32 camera pose; Ow = -Rcw^T tcw formed in float32 like Frame::UpdatePoseMatrices
    (src/Frame.cc:298-307)."""
    R = np.asarray(Rcw, dtype=np.float32).reshape(3, 3)
    t = np.asarray(tcw, dtype=np.float32).reshape(3)
    Ow = (-(R.T.astype(np.float32) @ t)).astype(np.float32)
    f = capi.FrustumFrame()
    f.Rcw[:] = [float(x) for x in R.reshape(9)]
    f.tcw[:] = [float(x) for x in t]
    f.Ow[:] = [float(x) for x in Ow]
    f.fx, f.fy, f.cx, f.cy, f.bf = fx, fy, cx, cy, bf
    f.min_x, f.max_x, f.min_y, f.max_y = bounds
    f.log_scale_factor, f.n_scale_levels, f.viewing_cos_limit = log_scale_factor, n_scale_levels, viewing_cos_limit
    if kb8 is not None:      # KannalaBrandt8 frame (monocular fisheye)
        f.fisheye = 1
        f.kb8[:] = [float(np.float32(k)) for k in kb8]
    return f


def frustum_args(pos, normal, min_dist, max_dist):
    """ctypes argument / result structs of osh_orb_frustum (also taken by the oracle) and the dict of output arrays."""
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    pos, normal, min_dist, max_dist = f32(pos), f32(normal), f32(min_dist), f32(max_dist)
    n = pos.shape[0]
    pts = capi.FrustumPoints()
    pts.n = n
    pts.pos, pts.normal = capi.ptr(pos, capi.c_float_p), capi.ptr(normal, capi.c_float_p)
    pts.min_dist, pts.max_dist = capi.ptr(min_dist, capi.c_float_p), capi.ptr(max_dist, capi.c_float_p)
    outs = dict(stage=np.zeros(n, np.uint8), proj_x=np.zeros(n, np.float32), proj_y=np.zeros(n, np.float32),
                proj_xr=np.zeros(n, np.float32), depth=np.zeros(n, np.float32), view_cos=np.zeros(n, np.float32),
                level=np.zeros(n, np.int32))
    res = capi.FrustumResult()
    res.stage = capi.ptr(outs["stage"], capi.c_uint8_p)
    for k in ("proj_x", "proj_y", "proj_xr", "depth", "view_cos"):
        setattr(res, k, capi.ptr(outs[k], capi.c_float_p))
    res.level = capi.ptr(outs["level"], capi.c_int32_p)
    return (pts, pos, normal, min_dist, max_dist), res, outs


_FUSE_OUTPUTS = (("stage", np.int32), ("u", np.float32), ("v", np.float32), ("ur", np.float32), ("level", np.int32), ("radius", np.float32),
                 ("n_candidates", np.int32), ("best_idx", np.int32), ("best_dist", np.int32))


def fuse_args(targets, points, fill=None):
    """The osh_fuse_target array, osh_fuse_points and osh_fuse_result of OrbMatcher.fuse_search for repeated calls, the arrays that
    keep their pointers alive and the dict of output arrays [n_targets, n]; fill = (int32 value, float32 value) presets them."""
    ct = (capi.FuseTarget * max(len(targets), 1))()
    keep = []
    for c, t in zip(ct, targets):
        sf, inv, log_sf = t.level_tables()
        c.Rcw[:] = [float(x) for x in np.asarray(t.Rcw, np.float32).reshape(9)]
        c.tcw[:] = [float(x) for x in np.asarray(t.tcw, np.float32)]
        c.Ow[:] = [float(x) for x in np.asarray(t.Ow, np.float32)]
        c.camera, c.fx, c.fy, c.cx, c.cy, c.bf = int(t.camera), t.fx, t.fy, t.cx, t.cy, t.bf
        c.kb8[:] = [float(x) for x in t.kb8]
        c.min_x, c.max_x, c.min_y, c.max_y = [float(x) for x in t.bounds]
        c.grid_min_x, c.grid_min_y = [float(x) for x in t.grid_min]
        c.cell_w_inv, c.cell_h_inv = [float(x) for x in t.cell_inv]
        c.cols, c.rows, c.n_levels, c.log_scale_factor, c.th = int(t.cols), int(t.rows), int(t.n_levels), float(log_sf), float(t.th)
        c.scale_factors[:len(sf)] = [float(x) for x in sf[:16]]
        c.inv_level_sigma2[:len(inv)] = [float(x) for x in inv[:16]]
        a = dict(key_xy=np.ascontiguousarray(t.key_xy, np.float32), key_octave=np.ascontiguousarray(t.key_octave, np.int32),
                 descriptors=np.ascontiguousarray(t.desc, np.uint8))
        if t.key_uright is not None:
            a["key_uright"] = np.ascontiguousarray(t.key_uright, np.float32)
        c.n_keys = int(a["key_octave"].shape[0])
        for name, arr in a.items():
            setattr(c, name, capi.ptr(arr, _POINTER[arr.dtype]))
        keep.append(a)
    cp = capi.FusePoints()
    a = dict(pos=np.ascontiguousarray(points.pos, np.float32), normal=np.ascontiguousarray(points.normal, np.float32),
             min_dist=np.ascontiguousarray(points.min_dist, np.float32), max_dist=np.ascontiguousarray(points.max_dist, np.float32),
             desc=np.ascontiguousarray(points.desc, np.uint8))
    if points.skip is not None:
        a["skip"] = np.ascontiguousarray(points.skip, np.uint8)
    cp.n = int(a["min_dist"].shape[0])
    for name, arr in a.items():
        setattr(cp, name, capi.ptr(arr, _POINTER[arr.dtype]))
    keep.append(a)
    ifill, ffill = (0, 0.0) if fill is None else fill
    out = {name: np.full((len(targets), cp.n), ifill if dt is np.int32 else ffill, dt) for name, dt in _FUSE_OUTPUTS}
    cr = capi.FuseResult()
    _wire_outputs(cr, out)
    return ct, cp, cr, keep, out


def fuse_cpu(targets, points, mode: int = capi.OSH_FUSE_CHI2, host_lib=None):
    """csrc/orb_fuse.h on the host in one thread (osh_host_fuse_search_cpu of the test library): the output dict of fuse_search and
    the wall time of the call in ms."""
    host_lib = host_lib or capi.load_host_library()
    ct, cp, cr, _keep, out = fuse_args(targets, points)
    ms = C.c_double(0)
    rc = host_lib.osh_host_fuse_search_cpu(len(targets), ct, C.byref(cp), mode, C.byref(cr), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"osh_host_fuse_search_cpu -> {rc}")
    return out, float(ms.value)
