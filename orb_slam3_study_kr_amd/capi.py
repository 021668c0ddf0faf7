"""ctypes mirror of include/orbslam3_hip.h and loader of the HIP shared library.

The product path has NO CPU fallback: if the gfx950 library is missing or fails
to load, :func:`load_library` raises.  (The CPU oracle under ``oracle/`` is test
infrastructure and is never imported from here.)  :func:`load_host_library`
loads the test-only library of the C++ host layer (include/orbslam3_hip_host.h).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent
LIB_PATH = PKG_DIR / "csrc" / "liborbslam3_hip.so"
HOST_LIB_PATH = PKG_DIR / "csrc" / "liborbslam3_hip_hosttest.so"

OSH_OK = 0
OSH_ERR_INVALID = -1
OSH_ERR_DEVICE = -2
OSH_ERR_UNSUPPORTED = -3
OSH_ERR_NO_DEVICE = -4
OSH_EDGE_MONO = 0
OSH_EDGE_STEREO = 1
OSH_EDGE_BODY = 2
OSH_EDGE_RIGHT = 2   # LocalInertialBA: EdgeMono(1), the right camera of a fisheye rig
OSH_LBA_MAX_TRACE = 128
OSH_K_COUNT = 11
KERNEL_NAMES = ["linearize", "pose_hess", "schur", "solve", "backsub", "residual", "control", "schur_reduce", "schur_cross", "lin_aux", "lin_pose"]

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)
c_int64_p = C.POINTER(C.c_int64)
c_float_p = C.POINTER(C.c_float)
c_uint32_p = C.POINTER(C.c_uint32)


class LbaProblem(C.Structure):
    """``osh_lba_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_free", C.c_int32), ("n_fixed", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
        ("pose_qt", c_double_p), ("pose_cam", c_double_p), ("points", c_double_p),
        ("edge_pose", c_int32_p), ("edge_point", c_int32_p), ("edge_kind", c_uint8_p),
        ("edge_obs", c_double_p), ("edge_info", c_double_p),
        ("huber_mono", C.c_double), ("huber_stereo", C.c_double),
        ("lambda_init", C.c_double), ("max_iterations", C.c_int32),
        ("stop_flag", c_uint8_p), ("kb8", c_double_p), ("cam2", c_double_p), ("trl", c_double_p),
    ]


class LbaResult(C.Structure):
    """``osh_lba_result`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("pose_qt", c_double_p), ("points", c_double_p), ("edge_chi2", c_double_p), ("edge_depth_pos", c_uint8_p),
        ("status", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32), ("n_trace", C.c_int32),
        ("chi2_trace", C.c_double * OSH_LBA_MAX_TRACE),
        ("lambda_trace", C.c_double * OSH_LBA_MAX_TRACE),
        ("trials_trace", C.c_int32 * OSH_LBA_MAX_TRACE),
        ("chi2_initial", C.c_double),
    ]


class PoseProblem(C.Structure):
    """``osh_pose_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_edges", C.c_int32), ("pose_qt", c_double_p), ("cam", c_double_p), ("points", c_double_p),
        ("edge_kind", c_uint8_p), ("edge_obs", c_double_p), ("edge_info", c_double_p),
        ("huber_mono", C.c_double), ("huber_stereo", C.c_double),
        ("chi2_mono", C.c_float * 4), ("chi2_stereo", C.c_float * 4), ("iterations", C.c_int32 * 4),
        ("kb8", c_double_p), ("cam2", c_double_p), ("trl", c_double_p),
    ]


class PoseResult(C.Structure):
    """``osh_pose_result`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("pose_qt", C.c_double * 7), ("outlier", c_uint8_p), ("edge_chi2", c_double_p),
        ("n_bad", C.c_int32), ("rounds", C.c_int32), ("iterations", C.c_int32 * 4), ("chi2_final", C.c_double * 4),
        ("status", C.c_int32),
    ]


class PgoProblem(C.Structure):
    """``osh_pgo_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_vertices", C.c_int32), ("estimate", c_double_p), ("fixed", c_uint8_p), ("fix_scale", c_uint8_p),
        ("n_edges", C.c_int32), ("edge_ij", C.POINTER(C.c_int32)), ("measurement", c_double_p),
        ("iterations", C.c_int32), ("lambda_init", C.c_double), ("solve_mode", C.c_int32),
    ]


class PgoResult(C.Structure):
    """``osh_pgo_result`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("estimate", c_double_p), ("iterations", C.c_int32), ("trials", C.c_int32),
        ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("envelope_entries", C.c_int64),
        ("envelope_tiles", C.c_int32), ("tall_columns", C.c_int32), ("status", C.c_int32),
    ]


class Pgo4Problem(C.Structure):
    """``osh_pgo4_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_vertices", C.c_int32), ("Rwb", c_double_p), ("twb", c_double_p), ("Rcw", c_double_p), ("tcw", c_double_p),
        ("Rcb", c_double_p), ("tcb", c_double_p), ("fixed", c_uint8_p), ("n_edges", C.c_int32), ("edge_ij", C.POINTER(C.c_int32)),
        ("dR", c_double_p), ("dt", c_double_p), ("info_diag", C.c_double * 6), ("iterations", C.c_int32), ("lambda_init", C.c_double),
        ("solve_mode", C.c_int32),
    ]


class Pgo4Result(C.Structure):
    """``osh_pgo4_result`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("Rcw", c_double_p), ("tcw", c_double_p), ("Rwb", c_double_p), ("twb", c_double_p), ("iterations", C.c_int32),
        ("trials", C.c_int32), ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_init_used", C.c_double),
        ("envelope_entries", C.c_int64), ("envelope_tiles", C.c_int32), ("tall_columns", C.c_int32), ("status", C.c_int32),
    ]


class Sim3Problem(C.Structure):
    """``osh_sim3_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_pairs", C.c_int32), ("S12", C.c_double * 8), ("fix_scale", C.c_int32), ("th2", C.c_float),
        ("cam1", C.c_double * 8), ("cam2", C.c_double * 8), ("kb8_1", C.c_int32), ("kb8_2", C.c_int32),
        ("X1c", c_double_p), ("X2c", c_double_p), ("obs1", c_double_p), ("obs2", c_double_p),
        ("info1", c_double_p), ("info2", c_double_p), ("iterations", C.c_int32 * 3),
    ]


class Sim3Result(C.Structure):
    """``osh_sim3_result`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("S12", C.c_double * 8), ("outlier1", c_uint8_p), ("outlier", c_uint8_p), ("chi2_12", c_double_p), ("chi2_21", c_double_p),
        ("n_bad", C.c_int32), ("n_in", C.c_int32), ("round2", C.c_int32), ("iterations", C.c_int32 * 2),
        ("chi2_end", C.c_double * 2), ("status", C.c_int32),
    ]


OSH_SIM3_MAX_ITERATIONS = 100   # the limit of every osh_sim3_problem.iterations entry
OSH_PGO_MAX_VERTICES = 4000
OSH_PGO_SOLVE_ENVELOPE = 0
OSH_PGO_SOLVE_DENSE = 1

OSH_PREINT_FLOATS = 72


class LibaProblem(C.Structure):
    """``osh_liba_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_opt", C.c_int32), ("n_fixed_imu", C.c_int32), ("n_fixed", C.c_int32),
        ("n_points", C.c_int32), ("n_edges", C.c_int32), ("n_links", C.c_int32),
        ("pose_Rcw", c_double_p), ("pose_tcw", c_double_p), ("pose_Rwb", c_double_p), ("pose_twb", c_double_p),
        ("Rcb", c_double_p), ("tcb", c_double_p), ("tbc", c_double_p), ("cam", c_double_p),
        ("vel", c_double_p), ("bias_g", c_double_p), ("bias_a", c_double_p), ("points", c_double_p),
        ("edge_pose", c_int32_p), ("edge_point", c_int32_p), ("edge_kind", c_uint8_p),
        ("edge_obs", c_double_p), ("edge_info", c_double_p),
        ("link_prev", c_int32_p), ("link_cur", c_int32_p), ("link_preint", c_float_p),
        ("link_info", c_double_p), ("link_info_g", c_double_p), ("link_info_a", c_double_p), ("link_robust", c_uint8_p),
        ("huber_mono", C.c_double), ("huber_stereo", C.c_double), ("huber_inertial", C.c_double),
        ("lambda_init", C.c_double), ("max_iterations", C.c_int32), ("kb8", c_double_p),
        ("cam2", c_double_p), ("trl", c_double_p), ("link_bias", c_int32_p),
    ]


class PoseiProblem(C.Structure):
    """``osh_posei_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("mode", C.c_int32), ("n_edges", C.c_int32), ("rec_init", C.c_int32),
        ("Rcw", c_double_p), ("tcw", c_double_p), ("Rwb", c_double_p), ("twb", c_double_p),
        ("vel", c_double_p), ("bias_g", c_double_p), ("bias_a", c_double_p),
        ("prev_Rwb", c_double_p), ("prev_twb", c_double_p), ("prev_vel", c_double_p), ("prev_bias_g", c_double_p), ("prev_bias_a", c_double_p),
        ("Rcb", c_double_p), ("tcb", c_double_p), ("tbc", c_double_p), ("cam", c_double_p), ("kb8", c_double_p), ("cam2", c_double_p),
        ("trl", c_double_p), ("preint", c_float_p), ("info_inertial", c_double_p), ("info_g", c_double_p), ("info_a", c_double_p),
        ("prior_Rwb", c_double_p), ("prior_twb", c_double_p), ("prior_vel", c_double_p), ("prior_bg", c_double_p), ("prior_ba", c_double_p),
        ("prior_H", c_double_p), ("points", c_double_p), ("edge_kind", c_uint8_p), ("edge_obs", c_double_p), ("edge_info", c_double_p),
        ("edge_close", c_uint8_p), ("huber_mono", C.c_double), ("huber_stereo", C.c_double), ("huber_prior", C.c_double),
        ("chi2_mono", C.c_float * 4), ("chi2_stereo", C.c_float * 4), ("iterations", C.c_int32 * 4),
    ]


class PoseiResult(C.Structure):
    """``osh_posei_result`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("Rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("Rwb", C.c_double * 9), ("twb", C.c_double * 3),
        ("vel", C.c_double * 3), ("bias_g", C.c_double * 3), ("bias_a", C.c_double * 3),
        ("outlier", c_uint8_p), ("edge_chi2", c_double_p),
        ("n_bad", C.c_int32), ("n_inliers", C.c_int32), ("rounds", C.c_int32), ("status", C.c_int32),
        ("H", C.c_double * 900),
    ]


class LibaResult(C.Structure):
    """``osh_liba_result`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("pose_Rcw", c_double_p), ("pose_tcw", c_double_p), ("pose_Rwb", c_double_p), ("pose_twb", c_double_p),
        ("vel", c_double_p), ("bias_g", c_double_p), ("bias_a", c_double_p), ("points", c_double_p),
        ("edge_chi2", c_double_p), ("edge_depth_pos", c_uint8_p),
        ("status", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32), ("n_trace", C.c_int32),
        ("chi2_trace", C.c_double * OSH_LBA_MAX_TRACE),
        ("lambda_trace", C.c_double * OSH_LBA_MAX_TRACE),
        ("trials_trace", C.c_int32 * OSH_LBA_MAX_TRACE),
        ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
    ]


class OrbBatch(C.Structure):
    """``osh_orb_batch`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_pairs", C.c_int32), ("n_query", C.c_int32), ("n_train", C.c_int32),
        ("query_desc", c_uint8_p), ("train_desc", c_uint8_p), ("train_level", c_int32_p),
        ("cand_off", c_int32_p), ("cand_idx", c_int32_p), ("pair_cand_base", c_int64_p),
    ]


class OrbGrid(C.Structure):
    """``osh_orb_grid`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("train_xy", c_float_p), ("train_uright", c_float_p), ("train_skip", c_uint8_p),
        ("min_x", C.c_float), ("min_y", C.c_float), ("cell_w_inv", C.c_float), ("cell_h_inv", C.c_float),
        ("cols", C.c_int32), ("rows", C.c_int32),
        ("query_window", c_float_p), ("query_levels", c_int32_p), ("query_uright", c_float_p),
    ]


class FrustumFrame(C.Structure):
    """``osh_frustum_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
        ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
        ("log_scale_factor", C.c_float), ("n_scale_levels", C.c_int32), ("viewing_cos_limit", C.c_float),
        ("fisheye", C.c_int32), ("kb8", C.c_float * 4),
    ]


class FrustumPoints(C.Structure):
    """``osh_frustum_points`` (include/orbslam3_hip.h)."""

    _fields_ = [("n", C.c_int32), ("pos", c_float_p), ("normal", c_float_p), ("min_dist", c_float_p), ("max_dist", c_float_p)]


class FrustumResult(C.Structure):
    """``osh_frustum_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("stage", c_uint8_p), ("proj_x", c_float_p), ("proj_y", c_float_p), ("proj_xr", c_float_p),
                ("depth", c_float_p), ("view_cos", c_float_p), ("level", c_int32_p)]


class StereoImage(C.Structure):
    """``osh_stereo_image`` (include/orbslam3_hip.h)."""

    _fields_ = [("data", c_uint8_p), ("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int64)]


class StereoFrame(C.Structure):
    """``osh_stereo_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_left", C.c_int32), ("n_right", C.c_int32),
        ("left_xy", c_float_p), ("left_octave", c_int32_p), ("left_desc", c_uint8_p),
        ("right_xy", c_float_p), ("right_octave", c_int32_p), ("right_desc", c_uint8_p),
        ("n_levels", C.c_int32), ("scale_factors", c_float_p), ("inv_scale_factors", c_float_p),
        ("left_pyramid", C.POINTER(StereoImage)), ("right_pyramid", C.POINTER(StereoImage)),
        ("bf", C.c_float), ("b", C.c_float),
    ]


class StereoResult(C.Structure):
    """``osh_stereo_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("u_right", c_float_p), ("depth", c_float_p), ("best_right", c_int32_p), ("hamming", c_int32_p),
                ("sad", c_int32_p), ("best_inc", c_int32_p), ("stage", c_uint8_p)]


class StereoResidentFrame(C.Structure):
    """``osh_stereo_resident_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_left", C.c_int32), ("n_right", C.c_int32),
        ("left_xy", c_float_p), ("left_octave", c_int32_p), ("left_desc", c_uint8_p),
        ("right_xy", c_float_p), ("right_octave", c_int32_p), ("right_desc", c_uint8_p),
        ("n_levels", C.c_int32), ("scale_factors", c_float_p), ("inv_scale_factors", c_float_p),
        ("left_token", C.c_uint64), ("right_token", C.c_uint64),
        ("bf", C.c_float), ("b", C.c_float),
    ]


class StereoPair(C.Structure):
    """``osh_stereo_pair`` (include/orbslam3_hip.h)."""

    _fields_ = [("bf", C.c_float), ("b", C.c_float)]


OSH_STEREO_MAX_LEVELS = 16
OSH_STEREO_NO_INC = -128
(OSH_STEREO_NO_CANDIDATE, OSH_STEREO_HAMMING, OSH_STEREO_RIGHT_GUARD, OSH_STEREO_PATCH, OSH_STEREO_BORDER_INC, OSH_STEREO_DELTA,
 OSH_STEREO_DISPARITY, OSH_STEREO_ACCEPTED, OSH_STEREO_MEDIAN_CUT) = range(9)


class FisheyeStereoFrame(C.Structure):
    """``osh_fisheye_stereo_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [
        ("n_left", C.c_int32), ("n_right", C.c_int32), ("mono_left", C.c_int32), ("mono_right", C.c_int32),
        ("left_xy", c_float_p), ("left_octave", c_int32_p), ("left_desc", c_uint8_p),
        ("right_xy", c_float_p), ("right_octave", c_int32_p), ("right_desc", c_uint8_p),
        ("n_levels", C.c_int32), ("level_sigma2", c_float_p),
        ("cam1", C.c_float * 8), ("cam2", C.c_float * 8), ("precision1", C.c_float), ("precision2", C.c_float),
        ("Rlr", C.c_float * 9), ("tlr", C.c_float * 3),
    ]


class FisheyeStereoResult(C.Structure):
    """``osh_fisheye_stereo_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("left_to_right", c_int32_p), ("right_to_left", c_int32_p), ("depth", c_float_p), ("p3d", c_float_p),
                ("best_right", c_int32_p), ("best_dist", c_int32_p), ("second_dist", c_int32_p), ("cos_parallax", c_float_p),
                ("stage", c_uint8_p)]


class Kb8Rig(C.Structure):
    """``osh_kb8_rig`` (include/orbslam3_hip.h)."""

    _fields_ = [("cam1", C.c_float * 8), ("cam2", C.c_float * 8), ("precision1", C.c_float), ("precision2", C.c_float),
                ("R12", C.c_float * 9), ("t12", C.c_float * 3)]


(OSH_FSTEREO_OUTSIDE, OSH_FSTEREO_NO_PAIR, OSH_FSTEREO_RATIO, OSH_FSTEREO_PARALLAX, OSH_FSTEREO_BEHIND_1, OSH_FSTEREO_BEHIND_2,
 OSH_FSTEREO_REPROJ_1, OSH_FSTEREO_REPROJ_2, OSH_FSTEREO_DEPTH, OSH_FSTEREO_ACCEPTED) = range(10)
OSH_FSTEREO_NO_COS = -2.0


class NewPointCamera(C.Structure):
    """``osh_newpoint_camera`` (include/orbslam3_hip.h)."""

    _fields_ = [("type", C.c_int32), ("precision", C.c_float), ("params", C.c_float * 8)]


class NewPointPose(C.Structure):
    """``osh_newpoint_pose`` (include/orbslam3_hip.h)."""

    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Rwc", C.c_float * 9), ("Ow", C.c_float * 3)]


class NewPointKeyFrame(C.Structure):
    """``osh_newpoint_keyframe`` (include/orbslam3_hip.h)."""

    _fields_ = [("pose", NewPointPose), ("right_pose", NewPointPose), ("has_camera2", C.c_int32), ("camera", NewPointCamera),
                ("camera2", NewPointCamera), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("invfx", C.c_float), ("invfy", C.c_float), ("mbf", C.c_float), ("mb", C.c_float), ("n_left", C.c_int32),
                ("n_keys", C.c_int32), ("n_levels", C.c_int32), ("level_sigma2", c_float_p), ("scale_factors", c_float_p)]


class NewPointSegment(C.Structure):
    """``osh_newpoint_segment`` (include/orbslam3_hip.h)."""

    _fields_ = [("kf1", NewPointKeyFrame), ("kf2", NewPointKeyFrame), ("ratio_factor", C.c_float), ("inertial", C.c_int32),
                ("far_points", C.c_int32), ("th_far_points", C.c_float), ("n_matches", C.c_int32),
                ("idx1", c_int32_p), ("idx2", c_int32_p), ("pt1", c_float_p), ("pt2", c_float_p), ("octave1", c_int32_p),
                ("octave2", c_int32_p), ("u_right1", c_float_p), ("u_right2", c_float_p), ("depth1", c_float_p), ("depth2", c_float_p)]


class NewPointResult(C.Structure):
    """``osh_newpoint_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("stage", c_uint8_p), ("source", c_uint8_p), ("cos_parallax", c_float_p), ("x3d", c_float_p)]


OSH_NEWPOINT_MAX_LEVELS, OSH_NEWPOINT_MAX_SEGMENTS, OSH_NEWPOINT_MAX_MATCHES = 16, 65535, 1 << 22
OSH_NEWPOINT_PINHOLE, OSH_NEWPOINT_KB8 = 0, 1
(OSH_NEWPOINT_LOW_PARALLAX, OSH_NEWPOINT_W_ZERO, OSH_NEWPOINT_NO_DEPTH, OSH_NEWPOINT_BEHIND_1, OSH_NEWPOINT_BEHIND_2,
 OSH_NEWPOINT_REPROJ_1, OSH_NEWPOINT_REPROJ_2, OSH_NEWPOINT_ZERO_DIST, OSH_NEWPOINT_FAR, OSH_NEWPOINT_SCALE,
 OSH_NEWPOINT_ACCEPTED) = range(11)
OSH_NEWPOINT_TRIANGULATED, OSH_NEWPOINT_STEREO_1, OSH_NEWPOINT_STEREO_2, OSH_NEWPOINT_NO_SOURCE = 0, 1, 2, 255


class TwoViewProblem(C.Structure):
    """``osh_two_view_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [("K", C.c_float * 9), ("sigma", C.c_float), ("n_iterations", C.c_int32), ("n_matches", C.c_int32),
                ("n_keys1", C.c_int32), ("n_keys2", C.c_int32), ("idx1", c_int32_p), ("idx2", c_int32_p), ("pt1", c_float_p),
                ("pt2", c_float_p), ("T1", C.c_float * 9), ("T2", C.c_float * 9), ("pn1", c_float_p), ("pn2", c_float_p),
                ("sets", c_int32_p)]


class TwoViewResult(C.Structure):
    """``osh_two_view_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("status", c_int32_p), ("T21", c_float_p), ("sh", c_float_p), ("sf", c_float_p), ("H21", c_float_p), ("F21", c_float_p),
                ("best_h", c_int32_p), ("best_f", c_int32_p), ("info", c_int32_p), ("inlier", c_uint8_p), ("x3d", c_float_p),
                ("triangulated", c_uint8_p), ("n_good", c_int32_p), ("parallax", c_float_p), ("debug_model_n", c_float_p),
                ("debug_model", c_float_p), ("debug_score", c_float_p), ("debug_R", c_float_p), ("debug_t", c_float_p)]


OSH_TWOVIEW_MAX_MATCHES, OSH_TWOVIEW_MAX_ITERATIONS, OSH_TWOVIEW_MAX_PROBLEMS = 8192, 1024, 4096
OSH_TWOVIEW_MAX_TOTAL_MATCHES, OSH_TWOVIEW_MAX_TOTAL_ITERATIONS = 524288, 262144
(OSH_TWOVIEW_ACCEPTED_H, OSH_TWOVIEW_ACCEPTED_F, OSH_TWOVIEW_NO_MODEL, OSH_TWOVIEW_H_DEGENERATE, OSH_TWOVIEW_NO_CLEAR_WINNER,
 OSH_TWOVIEW_TOO_FEW_POINTS, OSH_TWOVIEW_LOW_PARALLAX) = range(7)


class MlpnpProblem(C.Structure):
    """``osh_mlpnp_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [("camera_type", C.c_int32), ("camera", C.c_float * 8), ("n", C.c_int32), ("bearing", c_double_p), ("p3d", c_double_p),
                ("p2d", c_float_p), ("max_error", c_float_p), ("n_iterations", C.c_int32), ("sets", c_int32_p),
                ("min_inliers", C.c_int32), ("best_inliers_in", C.c_int32), ("best_refine_ok_in", C.c_int32)]


class MlpnpResult(C.Structure):
    """``osh_mlpnp_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("first_hit", c_int32_p), ("hit_record", c_int32_p), ("hit_pose", c_double_p), ("hit_count", c_int32_p),
                ("hit_mask", c_uint32_p), ("best_iteration", c_int32_p), ("best_count", c_int32_p), ("best_mask", c_uint32_p),
                ("best_pose", c_double_p), ("best_refine_ok", c_int32_p), ("n_records", c_int32_p), ("debug_pose", c_double_p),
                ("debug_count", c_int32_p), ("debug_record", c_int32_p), ("debug_record_count", c_int32_p),
                ("debug_record_pose", c_double_p)]


OSH_MLPNP_MAX_POINTS, OSH_MLPNP_MAX_ITERATIONS, OSH_MLPNP_MAX_PROBLEMS = 2048, 1024, 64
OSH_MLPNP_PINHOLE, OSH_MLPNP_KB8 = 0, 1


def ransac_mask_words(n: int) -> int:
    """OSH_MLPNP_MASK_WORDS(n) and OSH_SIM3R_MASK_WORDS(n): the words of one inlier mask over n correspondences."""
    return 2 * ((n + 63) // 64)


mlpnp_mask_words = sim3r_mask_words = ransac_mask_words   # the names of the two macros, for callers written against them


class Sim3rProblem(C.Structure):
    """``osh_sim3r_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [("camera_type1", C.c_int32), ("camera1", C.c_float * 8), ("camera_type2", C.c_int32), ("camera2", C.c_float * 8),
                ("fix_scale", C.c_int32), ("n", C.c_int32), ("x3dc1", c_float_p), ("x3dc2", c_float_p), ("p1im1", c_float_p),
                ("p2im2", c_float_p), ("max_error1", c_float_p), ("max_error2", c_float_p), ("n_iterations", C.c_int32),
                ("sets", c_int32_p), ("min_inliers", C.c_int32), ("best_inliers_in", C.c_int32)]


class Sim3rResult(C.Structure):
    """``osh_sim3r_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("first_hit", c_int32_p), ("n_records", c_int32_p), ("record", c_int32_p), ("record_count", c_int32_p),
                ("record_T", c_float_p), ("record_mask", c_uint32_p), ("best_iteration", c_int32_p), ("best_count", c_int32_p),
                ("debug_count", c_int32_p), ("debug_T", c_float_p)]


class HostSim3Scene(C.Structure):
    """``osh_host_sim3_scene`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("n_kf", C.c_int32), ("camera_type", C.c_int32 * 3), ("camera", (C.c_float * 8) * 3), ("Rcw", (C.c_float * 9) * 3),
                ("tcw", (C.c_float * 3) * 3), ("n_keys", C.c_int32 * 3), ("xy", c_float_p * 3), ("octave", c_int32_p * 3),
                ("n_levels", C.c_int32), ("level_sigma2", c_float_p), ("n_points", C.c_int32), ("world", c_float_p), ("bad", c_uint8_p),
                ("index_in_kf", c_int32_p), ("n1", C.c_int32), ("kf1_mp", c_int32_p), ("matched12", c_int32_p), ("matched_kf", c_int32_p),
                ("fix_scale", C.c_int32)]


OSH_SIM3R_MAX_POINTS, OSH_SIM3R_MAX_ITERATIONS, OSH_SIM3R_MAX_PROBLEMS = 4096, 1024, 64
OSH_SIM3R_PINHOLE, OSH_SIM3R_KB8 = 0, 1


class MapPointBatch(C.Structure):
    """``osh_mappoint_batch`` (include/orbslam3_hip.h)."""

    _fields_ = [("n_points", C.c_int32), ("entry_off", c_int32_p), ("desc", c_uint8_p), ("centre", c_int32_p), ("use_desc", c_uint8_p),
                ("n_centres", C.c_int32), ("centres", c_float_p), ("pos", c_float_p), ("ref_centre", c_int32_p),
                ("level_scale", c_float_p), ("top_scale", c_float_p)]


class MapPointResult(C.Structure):
    """``osh_mappoint_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("best_entry", c_int32_p), ("best_median", c_int32_p), ("normal", c_float_p), ("min_distance", c_float_p),
                ("max_distance", c_float_p)]


OSH_MAPPOINT_MAX_DESCRIPTORS, OSH_MAPPOINT_MAX_POINTS, OSH_MAPPOINT_MAX_ENTRIES = 256, 1 << 22, 1 << 25


class FuseTarget(C.Structure):
    """``osh_fuse_target`` (include/orbslam3_hip.h)."""

    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("camera", C.c_int32), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("kb8", C.c_float * 4), ("bf", C.c_float), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("grid_min_x", C.c_float), ("grid_min_y", C.c_float),
                ("cell_w_inv", C.c_float), ("cell_h_inv", C.c_float), ("cols", C.c_int32), ("rows", C.c_int32), ("n_levels", C.c_int32),
                ("log_scale_factor", C.c_float), ("scale_factors", C.c_float * 16), ("inv_level_sigma2", C.c_float * 16), ("th", C.c_float),
                ("n_keys", C.c_int32), ("key_xy", c_float_p), ("key_octave", c_int32_p), ("key_uright", c_float_p), ("descriptors", c_uint8_p)]


class FusePoints(C.Structure):
    """``osh_fuse_points`` (include/orbslam3_hip.h)."""

    _fields_ = [("n", C.c_int32), ("pos", c_float_p), ("normal", c_float_p), ("min_dist", c_float_p), ("max_dist", c_float_p),
                ("desc", c_uint8_p), ("skip", c_uint8_p)]


class FuseResult(C.Structure):
    """``osh_fuse_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("stage", c_int32_p), ("u", c_float_p), ("v", c_float_p), ("ur", c_float_p), ("level", c_int32_p), ("radius", c_float_p),
                ("n_candidates", c_int32_p), ("best_idx", c_int32_p), ("best_dist", c_int32_p)]


OSH_FUSE_MAX_TARGETS, OSH_FUSE_MAX_POINTS, OSH_FUSE_MAX_KEYS, OSH_FUSE_MAX_CELLS, OSH_FUSE_MAX_CELL_ENTRIES, OSH_FUSE_MAX_LEVELS = 1024, 1 << 20, 65536, 16384, 255, 16
OSH_FUSE_PINHOLE, OSH_FUSE_KB8 = 0, 1
OSH_FUSE_CHI2, OSH_FUSE_SIM3 = 0, 1
OSH_FUSE_SKIPPED, OSH_FUSE_BEHIND, OSH_FUSE_OUTSIDE, OSH_FUSE_DISTANCE, OSH_FUSE_ANGLE, OSH_FUSE_EMPTY, OSH_FUSE_SEARCHED = range(7)


class KfCullProblem(C.Structure):
    """``osh_kfcull_problem`` (include/orbslam3_hip.h)."""

    _fields_ = [("n_keyframes", C.c_int32), ("n_candidates", C.c_int32), ("redundant_th", C.c_float), ("cand_slot_off", c_int32_p),
                ("slot_point", c_int32_p), ("slot_level", c_int32_p), ("n_points", C.c_int32), ("point_n_obs", c_int32_p),
                ("point_bad", c_uint8_p), ("point_obs_off", c_int32_p), ("obs_kf", c_int32_p), ("obs_level", c_int32_p),
                ("obs_weight", c_int32_p)]


class KfCullResult(C.Structure):
    """``osh_kfcull_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("n_mps", c_int32_p), ("n_redundant", c_int32_p), ("redundant", c_uint8_p)]


class HostCullScene(C.Structure):
    """``osh_host_cull_scene`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("n_kf", C.c_int32), ("kf_id", c_int64_p), ("kf_n_slots", c_int32_p), ("kf_n_left", c_int32_p), ("kf_camera2", c_uint8_p),
                ("kf_th_depth", c_float_p), ("kf_timestamp", c_double_p), ("kf_not_erase", c_uint8_p), ("kf_bad", c_uint8_p),
                ("kf_imu_pos", c_float_p), ("kf_prev", c_int32_p), ("kf_next", c_int32_p), ("kf_has_preint", c_uint8_p),
                ("slot_point", c_int32_p), ("slot_octave", c_int32_p), ("slot_u_right", c_float_p), ("slot_depth", c_float_p),
                ("n_mp", C.c_int32), ("mp_n_obs", c_int32_p), ("mp_bad", c_uint8_p), ("init_kf_id", C.c_int64),
                ("keyframes_in_map", C.c_int32), ("imu_initialized", C.c_int32), ("inertial_ba2", C.c_int32)]


OSH_KFCULL_MAX_CANDIDATES, OSH_KFCULL_MAX_KEYFRAMES = 128, 4096
OSH_KFCULL_MAX_SLOTS, OSH_KFCULL_MAX_POINTS, OSH_KFCULL_MAX_OBSERVATIONS = 1 << 22, 1 << 22, 1 << 25


class FastFrame(C.Structure):
    """``osh_fast_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("n_levels", C.c_int32), ("pyramid", C.POINTER(StereoImage)), ("ini_th", C.c_int32), ("min_th", C.c_int32)]


class FastResult(C.Structure):
    """``osh_fast_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("capacity", C.c_int32), ("cell_capacity", C.c_int32), ("n_out", C.c_int32), ("n_cells", C.c_int32),
                ("pyramid_token", C.c_uint64), ("level_count", c_int32_p), ("xy", c_float_p), ("response", c_float_p),
                ("level", c_int32_p), ("cell", c_int32_p), ("used_min_th", c_uint8_p)]


class FastResidentFrame(C.Structure):
    """``osh_fast_resident_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("pyramid_token", C.c_uint64), ("ini_th", C.c_int32), ("min_th", C.c_int32)]


class OctreeList(C.Structure):
    """``osh_octree_list`` (include/orbslam3_hip.h)."""

    _fields_ = [("n", C.c_int32), ("xy", c_float_p), ("response", c_float_p), ("width", C.c_int32), ("height", C.c_int32),
                ("n_features", C.c_int32)]


class OctreeResult(C.Structure):
    """``osh_octree_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("capacity", C.c_int32), ("n_out", C.c_int32), ("status", C.c_int32), ("index", c_int32_p)]


OSH_OCTREE_MAX_FEATURES, OSH_OCTREE_MAX_CANDIDATES, OSH_OCTREE_MAX_ROOTS = 2048, 1 << 16, 64


class PyramidImage(C.Structure):
    """``osh_pyramid_image`` (include/orbslam3_hip.h)."""

    _fields_ = [("data", c_uint8_p), ("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int64)]


class PyramidFrame(C.Structure):
    """``osh_pyramid_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("image", StereoImage), ("n_levels", C.c_int32), ("inv_scale", c_float_p)]


class PyramidResult(C.Structure):
    """``osh_pyramid_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("pyramid_token", C.c_uint64), ("level_rows", c_int32_p), ("level_cols", c_int32_p), ("levels", C.POINTER(PyramidImage)),
                ("border", C.c_int32)]


class IcAngleFrame(C.Structure):
    """``osh_ic_angle_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("n_levels", C.c_int32), ("pyramid", C.POINTER(StereoImage)), ("pyramid_token", C.c_uint64), ("n", C.c_int32),
                ("xy", c_float_p), ("level", c_int32_p)]


class IcAngleResult(C.Structure):
    """``osh_ic_angle_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("angle", c_float_p), ("m10", c_int32_p), ("m01", c_int32_p)]


class ExtractFrame(C.Structure):
    """``osh_extract_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("image", StereoImage), ("n_levels", C.c_int32), ("inv_scale", c_float_p), ("scale", c_float_p), ("ini_th", C.c_int32),
                ("min_th", C.c_int32), ("n_features", c_int32_p), ("pattern", C.POINTER(C.c_int8)), ("blur_q8", C.POINTER(C.c_uint16))]


class ExtractResult(C.Structure):
    """``osh_extract_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("capacity", C.c_int32), ("n_out", C.c_int32), ("pyramid_token", C.c_uint64), ("level_count", c_int32_p), ("xy", c_float_p),
                ("level", c_int32_p), ("response", c_float_p), ("angle", c_float_p), ("size", c_float_p), ("descriptors", c_uint8_p),
                ("levels", C.POINTER(PyramidImage)), ("border", C.c_int32)]


class DescribeFrame(C.Structure):
    """``osh_describe_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("n_levels", C.c_int32), ("pyramid", C.POINTER(StereoImage)), ("pyramid_token", C.c_uint64), ("n", C.c_int32),
                ("xy", c_float_p), ("level", c_int32_p), ("angle", c_float_p), ("pattern", C.POINTER(C.c_int8)),
                ("blur_q8", C.POINTER(C.c_uint16))]


class DescribeResult(C.Structure):
    """``osh_describe_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("descriptors", c_uint8_p), ("cos_sin", c_float_p), ("blurred", c_uint8_p)]


class RectifyMapDesc(C.Structure):
    """``osh_rectify_map_desc`` (include/orbslam3_hip.h)."""

    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("map_x", c_float_p), ("map_x_stride", C.c_int64), ("map_y", c_float_p),
                ("map_y_stride", C.c_int64), ("src_rows", C.c_int32), ("src_cols", C.c_int32)]


class PrepareImage(C.Structure):
    """``osh_prepare_image`` (include/orbslam3_hip.h)."""

    _fields_ = [("data", c_uint8_p), ("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int64), ("channels", C.c_int32)]


class PrepareFrame(C.Structure):
    """``osh_prepare_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("image", PrepareImage), ("order", C.c_int32), ("map", C.c_void_p), ("out_rows", C.c_int32), ("out_cols", C.c_int32)]


class PrepareResult(C.Structure):
    """``osh_prepare_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("gray", c_uint8_p), ("gray_stride", C.c_int64)]


OSH_PREP_RGB, OSH_PREP_BGR = 0, 1
OSH_FAST_MAX_SIDE = 32768
OSH_FAST_AT_INI, OSH_FAST_AT_MIN, OSH_FAST_EMPTY = 0, 1, 2


class BowTree(C.Structure):
    """``osh_bow_tree`` (include/orbslam3_hip.h)."""

    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32), ("n", C.c_int32),
                ("parent", c_int32_p), ("is_leaf", c_uint8_p), ("desc", c_uint8_p), ("weight", c_double_p)]


class BowFrame(C.Structure):
    """``osh_bow_frame`` (include/orbslam3_hip.h)."""

    _fields_ = [("n", C.c_int32), ("desc", c_uint8_p)]


class BowResult(C.Structure):
    """``osh_bow_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("n_words", c_int32_p), ("word_id", c_int32_p), ("word_value", c_double_p), ("n_nodes", c_int32_p),
                ("node_id", c_int32_p), ("node_start", c_int32_p), ("node_feat", c_int32_p), ("feat_word", c_int32_p),
                ("feat_node", c_int32_p), ("feat_dist", c_int32_p)]


class BowDbQuery(C.Structure):
    """``osh_bow_db_query`` (include/orbslam3_hip.h)."""

    _fields_ = [("n", C.c_int32), ("word_id", c_int32_p), ("value", c_double_p), ("n_excluded", C.c_int32),
                ("excluded", C.POINTER(C.c_uint64))]


class BowDbResult(C.Structure):
    """``osh_bow_db_result`` (include/orbslam3_hip.h)."""

    _fields_ = [("capacity", C.c_int32), ("max_common", c_int32_p), ("min_common", c_int32_p), ("n_rows", c_int32_p),
                ("handle", C.POINTER(C.c_uint64)), ("common", c_int32_p), ("first_word", c_int32_p), ("scored", c_uint8_p),
                ("score", c_double_p)]


OSH_BOW_MAX_K, OSH_BOW_MAX_L, OSH_BOW_MAX_FEATURES = 20, 10, 16384
OSH_BOW_DB_MAX_ROWS = 1 << 20
OSH_BOW_TF_IDF, OSH_BOW_TF, OSH_BOW_IDF, OSH_BOW_BINARY = range(4)
(OSH_BOW_L1_NORM, OSH_BOW_L2_NORM, OSH_BOW_CHI_SQUARE, OSH_BOW_KL, OSH_BOW_BHATTACHARYYA, OSH_BOW_DOT_PRODUCT) = range(6)


def ptr(a, typ):
    """Pointer of ctypes type `typ` to the data of numpy array `a` (None -> NULL)."""
    if a is None:
        return C.cast(None, typ)
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(typ)


# Every symbol include/orbslam3_hip.h declares, with its signature.
_SIGNATURES = {
    "osh_last_error": (C.c_char_p, []),
    "osh_version": (C.c_char_p, []),
    "osh_device_count": (C.c_int, []),
    "osh_lba_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "osh_lba_destroy": (None, [C.c_void_p]),
    "osh_lba_upload": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LbaProblem)]),
    "osh_lba_optimize": (C.c_int, [C.c_void_p]),
    "osh_lba_download": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LbaResult)]),
    "osh_lba_solve": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LbaProblem), C.POINTER(LbaResult)]),
    "osh_lba_linearize": (C.c_int, [C.c_void_p, C.c_int32] + [c_double_p] * 7),
    "osh_lba_debug_trial": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, c_double_p, c_double_p, c_double_p]),
    "osh_liba_solve": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LibaProblem), C.POINTER(LibaResult)]),
    "osh_lba_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "osh_lba_get_profile": (C.c_int, [C.c_void_p, c_int64_p, c_double_p]),
    "osh_lba_kernel_name": (C.c_char_p, [C.c_int]),
    "osh_pose_optimize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PoseProblem), C.POINTER(PoseResult)]),
    "osh_lba_get_plan_stats": (C.c_int, [C.c_void_p, c_int64_p]),
    "osh_lba_get_upload_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_lba_get_pack_profile": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_lba_set_pack_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "osh_lba_pack_compare": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LbaProblem), c_int64_p]),
    "osh_lba_schur_plan_stats": (C.c_int, [C.POINTER(LbaProblem), c_int64_p]),
    "osh_lba_schur_plan_stats_cut": (C.c_int, [C.POINTER(LbaProblem), C.c_int, c_int64_p]),
    "osh_lba_pack_cuts": (C.c_int, [C.c_int32, C.c_int, c_int32_p]),
    "osh_lba_pack_check_cut": (C.c_int, [C.c_int32, C.POINTER(LbaProblem), C.c_int32, C.c_int32, C.c_int32, c_int64_p, c_double_p]),
    "osh_lba_schur_plan_shapes": (C.c_int, [C.POINTER(LbaProblem), C.c_int, c_int64_p, c_int64_p]),
    "osh_lba_schur_block_list": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, c_int32_p]),
    "osh_lba_pack_check": (C.c_int, [C.c_int32, C.POINTER(LbaProblem), C.c_int32, c_int64_p, c_double_p]),
    "osh_liba_pack_check": (C.c_int, [C.c_int32, C.POINTER(LibaProblem), c_int64_p]),
    "osh_lm_control_check": (C.c_int, [C.c_double, C.c_double, C.c_int32, c_double_p, c_int32_p, c_double_p, c_double_p, c_double_p,
                                       c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "osh_lba_get_solver": (C.c_int, [C.c_void_p, c_int32_p]),
    "osh_lba_solve_plan_check": (C.c_int, [C.c_int32] * 5 + [c_int32_p]),
    "osh_orb_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "osh_orb_destroy": (None, [C.c_void_p]),
    "osh_orb_upload": (C.c_int, [C.c_void_p, C.POINTER(OrbBatch)]),
    "osh_orb_upload_grid": (C.c_int, [C.c_void_p, C.POINTER(OrbBatch), C.POINTER(OrbGrid)]),
    "osh_orb_frustum": (C.c_int, [C.c_void_p, C.POINTER(FrustumFrame), C.POINTER(FrustumPoints), C.POINTER(FrustumResult)]),
    "osh_posei_optimize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PoseiProblem), C.POINTER(PoseiResult)]),
    "osh_posei_linearize": (C.c_int, [C.c_void_p, C.POINTER(PoseiProblem), c_double_p, c_double_p]),
    "osh_orb_match": (C.c_int, [C.c_void_p]),
    "osh_orb_match_local_points": (C.c_int, [C.c_void_p, C.c_float, C.c_int32, c_uint8_p, c_uint8_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "osh_orb_download": (C.c_int, [C.c_void_p] + [c_int32_p] * 6),
    "osh_orb_get_profile": (C.c_int, [C.c_void_p, c_int64_p, c_double_p]),
    "osh_orb_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "osh_liba_get_profile": (C.c_int, [C.POINTER(C.c_int32), c_int64_p]),
    "osh_liba_linearize": (C.c_int, [C.c_void_p, C.POINTER(LibaProblem), c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p]),
    "osh_liba_inertial_edges": (C.c_int, [C.c_void_p, C.POINTER(LibaProblem), c_double_p, c_double_p, c_double_p]),
    "osh_liba_debug_trial": (C.c_int, [C.c_void_p, C.POINTER(LibaProblem), C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "osh_orb_list_distances": (C.c_int, [C.c_void_p, c_int32_p]),
    "osh_orb_get_resolve_profile": (C.c_int, [C.c_void_p, c_int64_p, c_double_p]),
    "osh_orb_distance_matrix": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_uint8_p, c_uint8_p, c_int32_p]),
    "osh_orb_stereo_match": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(StereoFrame), C.POINTER(StereoResult)]),
    "osh_orb_stereo_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_stereo_set_row_search": (C.c_int, [C.c_void_p, C.c_int32]),
    "osh_orb_stereo_match_resident": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(StereoResidentFrame), C.POINTER(StereoResult)]),
    "osh_orb_fisheye_stereo_match": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(FisheyeStereoFrame), C.POINTER(FisheyeStereoResult)]),
    "osh_orb_fisheye_stereo_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_kb8_triangulate": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Kb8Rig)] + [c_float_p] * 7),
    "osh_orb_triangulate_new_points": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(NewPointSegment), C.POINTER(NewPointResult)]),
    "osh_orb_newpoint_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_two_view_reconstruct": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(TwoViewProblem), C.POINTER(TwoViewResult)]),
    "osh_orb_two_view_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_mlpnp_solve": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MlpnpProblem), C.POINTER(MlpnpResult)]),
    "osh_orb_mlpnp_check_inliers": (C.c_int, [C.c_void_p, C.POINTER(MlpnpProblem), C.c_int32, c_double_p, c_int32_p, c_uint32_p]),
    "osh_orb_mlpnp_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_sim3_ransac": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Sim3rProblem), C.POINTER(Sim3rResult)]),
    "osh_orb_sim3_ransac_check_inliers": (C.c_int, [C.c_void_p, C.POINTER(Sim3rProblem), C.c_int32, c_float_p, c_int32_p, c_uint32_p]),
    "osh_orb_sim3_ransac_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_refresh_map_points": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MapPointBatch), C.POINTER(MapPointResult)]),
    "osh_orb_refresh_map_points_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_fuse_search": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(FuseTarget), C.POINTER(FusePoints), C.c_int32, C.POINTER(FuseResult)]),
    "osh_orb_fuse_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_keyframe_cull_stage": (C.c_int, [C.c_void_p, C.POINTER(KfCullProblem)]),
    "osh_orb_keyframe_cull_count": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.c_int32, C.POINTER(KfCullResult)]),
    "osh_orb_keyframe_cull_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_fast_detect": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(FastFrame), C.POINTER(FastResult)]),
    "osh_orb_ic_angle": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(IcAngleFrame), C.POINTER(IcAngleResult)]),
    "osh_orb_fast_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_ic_angle_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_fast_detect_resident": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(FastResidentFrame), C.POINTER(FastResult)]),
    "osh_orb_octree_distribute": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(OctreeList), C.POINTER(OctreeResult)]),
    "osh_orb_octree_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_pyramid_build": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PyramidFrame), C.POINTER(PyramidResult)]),
    "osh_orb_pyramid_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_describe": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(DescribeFrame), C.POINTER(DescribeResult)]),
    "osh_orb_describe_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_extract": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(ExtractFrame), C.POINTER(ExtractResult)]),
    "osh_orb_extract_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_rectify_map_create": (C.c_int, [C.c_int, C.POINTER(RectifyMapDesc), C.POINTER(C.c_void_p)]),
    "osh_rectify_map_destroy": (None, [C.c_void_p]),
    "osh_orb_prepare": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PrepareFrame), C.POINTER(PrepareResult)]),
    "osh_orb_extract_raw": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PrepareFrame), C.POINTER(ExtractFrame), C.POINTER(ExtractResult),
                                      C.POINTER(PrepareResult)]),
    "osh_orb_prepare_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_orb_extract_stereo": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PrepareFrame), C.POINTER(ExtractFrame), C.POINTER(StereoPair),
                                         C.POINTER(ExtractResult), C.POINTER(StereoResult)]),
    "osh_orb_extract_stereo_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_bow_tree_check": (C.c_int, [C.POINTER(BowTree)]),
    "osh_bow_vocab_create": (C.c_int, [C.c_int, C.POINTER(BowTree), C.POINTER(C.c_void_p)]),
    "osh_bow_vocab_destroy": (None, [C.c_void_p]),
    "osh_orb_bow_transform": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(BowFrame), C.POINTER(BowResult)]),
    "osh_orb_bow_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_bow_db_create": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_void_p)]),
    "osh_bow_db_destroy": (None, [C.c_void_p]),
    "osh_bow_db_add": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_double_p, C.POINTER(C.c_uint64)]),
    "osh_bow_db_erase": (C.c_int, [C.c_void_p, C.c_uint64]),
    "osh_bow_db_clear": (C.c_int, [C.c_void_p]),
    "osh_bow_db_info": (C.c_int, [C.c_void_p, c_int64_p]),
    "osh_orb_bow_db_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(BowDbQuery), C.POINTER(BowDbResult)]),
    "osh_orb_bow_db_get_times": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_pgo_solve": (C.c_int, [C.c_void_p, C.POINTER(PgoProblem), C.POINTER(PgoResult)]),
    "osh_pgo_linearize": (C.c_int, [C.c_void_p, C.POINTER(PgoProblem), c_double_p, c_double_p, c_double_p]),
    "osh_pgo4_solve": (C.c_int, [C.c_void_p, C.POINTER(Pgo4Problem), C.POINTER(Pgo4Result)]),
    "osh_pgo4_linearize": (C.c_int, [C.c_void_p, C.POINTER(Pgo4Problem), c_double_p, c_double_p, c_double_p]),
    "osh_sim3_optimize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Sim3Problem), C.POINTER(Sim3Result)]),
    "osh_sim3_linearize": (C.c_int, [C.c_void_p, C.POINTER(Sim3Problem), c_double_p, c_double_p, c_double_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# include/orbslam3_hip_host.h (C wrappers of the C++ host layer)
c_float_p = C.POINTER(C.c_float)


class HostStereoInput(C.Structure):
    """``osh_host_stereo_input`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("n_left", C.c_int32), ("n_right", C.c_int32),
        ("left_xy", c_float_p), ("left_octave", c_int32_p), ("left_desc", c_uint8_p),
        ("right_xy", c_float_p), ("right_octave", c_int32_p), ("right_desc", c_uint8_p),
        ("n_levels", C.c_int32), ("scale_factors", c_float_p), ("inv_scale_factors", c_float_p),
        ("left_rows", c_int32_p), ("left_cols", c_int32_p), ("right_rows", c_int32_p), ("right_cols", c_int32_p),
        ("left_pixels", c_uint8_p), ("right_pixels", c_uint8_p),
        ("bf", C.c_float), ("b", C.c_float),
    ]


class HostFisheyeInput(C.Structure):
    """``osh_host_fisheye_input`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("n_left", C.c_int32), ("n_right", C.c_int32), ("mono_left", C.c_int32), ("mono_right", C.c_int32),
        ("left_xy", c_float_p), ("left_octave", c_int32_p), ("left_desc", c_uint8_p),
        ("right_xy", c_float_p), ("right_octave", c_int32_p), ("right_desc", c_uint8_p),
        ("n_levels", C.c_int32), ("level_sigma2", c_float_p),
        ("cam1", C.c_float * 8), ("cam2", C.c_float * 8), ("precision1", C.c_float), ("precision2", C.c_float),
        ("Rlr", C.c_float * 9), ("tlr", C.c_float * 3),
    ]


class HostNewPointKf(C.Structure):
    """``osh_host_newpoint_kf`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("n", C.c_int32), ("n_left", C.c_int32), ("xy", c_float_p), ("octave", c_int32_p), ("desc", c_uint8_p),
                ("u_right", c_float_p), ("depth", c_float_p), ("has_mp", c_uint8_p), ("mp_pos", c_float_p), ("n_nodes", C.c_int32),
                ("node_id", c_int32_p), ("node_off", c_int32_p), ("node_feat", c_int32_p), ("pose_qt", C.c_float * 7),
                ("trl_qt", C.c_float * 7), ("camera_kb8", C.c_int32), ("camera", C.c_float * 8), ("has_camera2", C.c_int32),
                ("camera2", C.c_float * 8), ("mbf", C.c_float), ("mb", C.c_float), ("n_levels", C.c_int32),
                ("scale_factor", C.c_float), ("prev", C.c_int32)]


class HostNewPointScene(C.Structure):
    """``osh_host_newpoint_scene`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("n_kf", C.c_int32), ("kf", C.POINTER(HostNewPointKf)), ("n_neighbours", C.c_int32), ("neighbours", c_int32_p),
                ("monocular", C.c_int32), ("inertial", C.c_int32), ("far_points", C.c_int32), ("th_far_points", C.c_float),
                ("recently_lost", C.c_int32), ("inertial_ba2", C.c_int32), ("new_keyframe_waiting", C.c_int32)]


class HostOrbExtractorInput(C.Structure):
    """``osh_host_orbextractor_input`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32), ("ini_th", C.c_int32),
                ("min_th", C.c_int32), ("n_images", C.c_int32), ("rows", c_int32_p), ("cols", c_int32_p), ("pixels", c_uint8_p),
                ("border", C.c_int32)]


class HostOrbExtractorOutput(C.Structure):
    """``osh_host_orbextractor_output`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("capacity", C.c_int32), ("cand_capacity", C.c_int32), ("level_count", c_int32_p), ("xy", c_float_p),
                ("response", c_float_p), ("angle", c_float_p), ("size", c_float_p), ("octave", c_int32_p),
                ("cand_level_count", c_int32_p), ("cand_xy", c_float_p), ("cand_response", c_float_p), ("cand_args", c_int32_p),
                ("features_per_level", c_int32_p), ("scale_factors", c_float_p)]


class HostExtractInput(C.Structure):
    """``osh_host_extract_input`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32), ("ini_th", C.c_int32),
                ("min_th", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("pixels", c_uint8_p), ("lapping", C.c_int32 * 2)]


class HostExtractOutput(C.Structure):
    """``osh_host_extract_output`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("capacity", C.c_int32), ("pixel_capacity", C.c_int32), ("level_rows", c_int32_p), ("level_cols", c_int32_p),
                ("pyramid", c_uint8_p), ("level_count", c_int32_p), ("level_xy", c_float_p), ("level_angle", c_float_p),
                ("xy", c_float_p), ("angle", c_float_p), ("size", c_float_p), ("response", c_float_p), ("octave", c_int32_p),
                ("descriptors", c_uint8_p), ("ret", c_int32_p), ("desc_rows", c_int32_p), ("pixels_needed", c_int32_p),
                ("call_ms", c_double_p)]


class HostRawImage(C.Structure):
    """``osh_host_raw_image`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("channels", C.c_int32), ("pixels", c_uint8_p), ("rgb", C.c_int32),
                ("map_rows", C.c_int32), ("map_cols", C.c_int32), ("map_x", c_float_p), ("map_y", c_float_p), ("new_rows", C.c_int32),
                ("new_cols", C.c_int32)]


class HostPyramidOutput(C.Structure):
    """``osh_host_pyramid_output`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("capacity", C.c_int32), ("pixel_capacity", C.c_int32), ("level_rows", c_int32_p), ("level_cols", c_int32_p),
                ("bordered", c_uint8_p), ("pixels_needed", c_int32_p), ("built_token", C.POINTER(C.c_uint64)), ("level_count", c_int32_p),
                ("xy", c_float_p), ("angle", c_float_p), ("response", c_float_p), ("hand_level_count", c_int32_p), ("hand_xy", c_float_p),
                ("hand_angle", c_float_p), ("hand_response", c_float_p)]


_HOST_SIGNATURES = {
    "osh_host_orb_pyramid_cpu": (C.c_int, [C.c_int32, C.POINTER(PyramidFrame), C.POINTER(PyramidResult), c_double_p]),
    "osh_host_orb_prepare_cpu": (C.c_int, [C.c_int32, C.POINTER(PrepareFrame), C.POINTER(C.POINTER(RectifyMapDesc)), C.POINTER(PrepareResult),
                                           c_double_p]),
    "osh_host_orbextractor_compute_pyramid": (C.c_int, [C.POINTER(HostExtractInput), C.POINTER(HostPyramidOutput)]),
    "osh_host_orb_describe_cpu": (C.c_int, [C.c_int32, C.POINTER(DescribeFrame), C.POINTER(DescribeResult), c_double_p]),
    "osh_host_brief_gaussian_q8": (C.c_int, [C.c_int32, C.c_double, C.POINTER(C.c_uint16)]),
    "osh_host_brief_reach": (C.c_int, [C.POINTER(C.c_int8)]),
    "osh_host_orbextractor_pattern": (C.c_int, [C.POINTER(C.c_int8)]),
    "osh_host_orbextractor_extract": (C.c_int, [C.POINTER(HostExtractInput), C.POINTER(HostExtractOutput)]),
    "osh_host_orbextractor_extract_batch": (C.c_int, [C.c_int32, C.POINTER(HostExtractInput), C.POINTER(HostExtractOutput), C.c_int32,
                                                      C.POINTER(C.c_uint64)]),
    "osh_host_frame_extract_and_match_stereo": (C.c_int, [C.POINTER(HostExtractInput), C.POINTER(HostRawImage), C.c_float, C.c_float, C.c_int32,
                                                          C.POINTER(HostExtractOutput), C.POINTER(C.c_uint64), C.c_int32, c_float_p, c_float_p,
                                                          c_int32_p, C.POINTER(c_uint8_p), c_int32_p, c_int32_p, c_int32_p, C.POINTER(C.c_double)]),
    "osh_host_orbextractor_extract_batch_raw": (C.c_int, [C.c_int32, C.POINTER(HostExtractInput), C.POINTER(HostRawImage),
                                                          C.POINTER(HostExtractOutput), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(c_uint8_p),
                                                          c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_orb_fast_cpu": (C.c_int, [C.c_int32, C.POINTER(FastFrame), C.POINTER(FastResult), c_double_p]),
    "osh_host_orb_ic_angle_cpu": (C.c_int, [C.c_int32, C.POINTER(IcAngleFrame), C.POINTER(IcAngleResult), c_double_p]),
    "osh_host_orb_fast_level_cells": (C.c_int, [C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
    "osh_host_orb_octree_cpu": (C.c_int, [C.c_int32, C.POINTER(OctreeList), C.POINTER(OctreeResult), c_double_p]),
    "osh_host_orbextractor_distribute_device": (C.c_int, [C.POINTER(OctreeList), C.c_int32, c_int32_p, c_float_p, c_float_p, c_int32_p]),
    "osh_host_orbextractor_compute_keypoints": (C.c_int, [C.POINTER(HostOrbExtractorInput), C.POINTER(HostOrbExtractorOutput)]),
    "osh_host_create_new_map_points": (C.c_int, [C.POINTER(HostNewPointScene), C.c_int32, c_int32_p, c_int32_p, c_int32_p, c_float_p,
                                                 c_int32_p, c_int32_p, c_float_p]),
    "osh_host_compute_fisheye_stereo_matches": (C.c_int, [C.POINTER(HostFisheyeInput), C.c_int32, c_int32_p, c_int32_p, c_float_p, c_float_p, c_float_p]),
    "osh_host_kb8_triangulate_cpu": (C.c_int, [C.c_int32, C.POINTER(Kb8Rig)] + [c_float_p] * 7),
    "osh_host_newpoint_triangulate_cpu": (C.c_int, [C.c_int32, C.POINTER(NewPointSegment), C.POINTER(NewPointResult), c_double_p]),
    "osh_host_mlpnp_cpu": (C.c_int, [C.c_int32, C.POINTER(MlpnpProblem), C.POINTER(MlpnpResult), c_double_p]),
    "osh_host_mlpnp_check_inliers": (C.c_int, [C.POINTER(MlpnpProblem), C.c_int32, c_double_p, c_int32_p, c_uint32_p]),
    "osh_host_mlpnp_nullspace": (C.c_int, [c_double_p, c_double_p]),
    "osh_host_mlpnp_rank": (C.c_int, [c_double_p]),
    "osh_host_mlpnp_null_vector": (C.c_int, [c_double_p, C.c_int32, c_double_p]),
    "osh_host_mlpnp_compute_pose": (C.c_int, [C.c_int32, c_double_p, c_double_p, c_double_p, c_int32_p]),
    "osh_host_mlpnp_gauss_newton": (C.c_int, [C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int32, c_int32_p]),
    "osh_host_mlpnp_ransac_parameters": (C.c_int, [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_float, c_int32_p]),
    "osh_host_mlpnp_solver_create": (C.c_void_p, [C.c_int32, c_float_p, C.c_int32, c_float_p, c_int32_p, C.c_int32, c_float_p, C.c_int32, c_float_p,
                                                  c_uint8_p]),
    "osh_host_mlpnp_solver_destroy": (None, [C.c_void_p]),
    "osh_host_mlpnp_solver_set_ransac": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float]),
    "osh_host_mlpnp_solver_state": (C.c_int, [C.c_void_p, c_int32_p]),
    "osh_host_mlpnp_solver_iterate": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, c_uint8_p, c_uint8_p, c_int32_p,
                                                c_uint8_p, c_float_p]),
    "osh_host_mlpnp_solver_prepare": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p]),
    "osh_host_mlpnp_solver_replay": (C.c_int, [C.c_void_p, c_int32_p, c_double_p, c_uint32_p, c_double_p, c_uint32_p, C.c_int32, c_uint8_p, c_int32_p,
                                               c_uint8_p, c_float_p]),
    "osh_host_mlpnp_replay": (C.c_int, [C.c_int32, c_int32_p, C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_sim3r_cpu": (C.c_int, [C.c_int32, C.POINTER(Sim3rProblem), C.POINTER(Sim3rResult), c_double_p]),
    "osh_host_sim3r_check_inliers": (C.c_int, [C.POINTER(Sim3rProblem), C.c_int32, c_float_p, c_int32_p, c_uint32_p]),
    "osh_host_sim3r_compute_sim3": (C.c_int, [c_float_p, c_float_p, C.c_int32, c_float_p]),
    "osh_host_sim3r_scan": (C.c_int, [C.c_int32, c_int32_p, C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
    "osh_host_sim3r_max_iterations": (C.c_int, [C.c_int32, C.c_double, C.c_int32, C.c_int32]),
    "osh_host_sim3_solver_create": (C.c_void_p, [C.POINTER(HostSim3Scene)]),
    "osh_host_sim3_solver_destroy": (None, [C.c_void_p]),
    "osh_host_sim3_solver_set_ransac": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32]),
    "osh_host_sim3_solver_state": (C.c_int, [C.c_void_p, c_int32_p]),
    "osh_host_sim3_solver_pack": (C.c_int, [C.c_void_p] + [c_float_p] * 6 + [c_int32_p]),
    "osh_host_sim3_solver_best": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_uint8_p]),
    "osh_host_sim3_solver_iterate": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, c_uint8_p, c_int32_p, c_uint8_p,
                                               c_uint8_p, c_float_p]),
    "osh_host_sim3_solver_prepare": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p]),
    "osh_host_sim3_solver_keep": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_float_p, c_uint32_p]),
    "osh_host_sim3_solver_replay": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_uint8_p, c_int32_p, c_uint8_p, c_uint8_p, c_float_p]),
    "osh_host_two_view_cpu": (C.c_int, [C.c_int32, C.POINTER(TwoViewProblem), C.POINTER(TwoViewResult), c_double_p]),
    "osh_host_two_view_normalize": (C.c_int, [C.c_int32, c_float_p, c_float_p, c_float_p]),
    "osh_host_two_view_decide": (C.c_int, [C.c_int32, C.c_int32, c_int32_p, c_float_p, c_int32_p]),
    "osh_host_two_view_motion": (C.c_int, [C.c_int32, c_float_p, c_float_p, c_float_p, c_float_p]),
    "osh_host_two_view_reconstruct": (C.c_int, [C.c_int32, c_float_p, C.c_float, C.c_int32, C.c_int32, c_float_p, C.c_int32, c_float_p,
                                                c_int32_p, c_float_p, c_float_p, c_int32_p, c_uint8_p, c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_graph_create": (C.c_void_p, [C.c_int32, c_int64_p, c_float_p, c_float_p, c_float_p, C.c_int32, C.c_int32, c_int64_p,
                                           c_float_p, C.c_int32, c_int32_p, c_int32_p, c_float_p, c_int32_p, C.c_int64, C.c_int32]),
    "osh_host_graph_destroy": (None, [C.c_void_p]),
    "osh_host_last_call_ms": (C.c_double, []),
    "osh_host_search_by_sim3": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p, C.c_float, C.c_int32, c_float_p, c_uint8_p, c_float_p, c_uint8_p, c_int32_p,
                                          C.c_int32, c_float_p, c_uint8_p, c_float_p, c_uint8_p, c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_graph_set_fisheye": (None, [C.c_void_p, c_float_p]),
    "osh_host_graph_set_rig": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int32, c_int32_p, c_int32_p, c_float_p, c_int32_p]),
    "osh_host_last_pack_rig": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "osh_host_last_pack_kb8": (C.c_int, [C.c_void_p, c_double_p]),
    "osh_host_graph_set_covisible": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p]),
    "osh_host_pack_lba": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_double_p, c_double_p, c_double_p, c_int32_p, c_int32_p,
                                    c_uint8_p, c_double_p, c_double_p, c_int64_p, c_int64_p]),
    "osh_host_run_lba": (C.c_int, [C.c_void_p, C.c_int32, c_uint8_p, c_int32_p]),
    "osh_host_get_kf_pose": (None, [C.c_void_p, C.c_int32, c_float_p]),
    "osh_host_get_mp_pos": (None, [C.c_void_p, C.c_int32, c_float_p]),
    "osh_host_mp_num_observations": (C.c_int, [C.c_void_p, C.c_int32]),
    "osh_host_mp_is_bad": (C.c_int, [C.c_void_p, C.c_int32]),
    "osh_host_kf_num_matches": (C.c_int, [C.c_void_p, C.c_int32]),
    "osh_host_kf_observes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "osh_host_map_change_index": (C.c_int, [C.c_void_p]),
    "osh_host_kf_pose_sets": (C.c_int, [C.c_void_p, C.c_int32]),
    "osh_host_graph_set_inertial": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]),
    "osh_host_pack_liba": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(LibaProblem), c_int64_p, c_int64_p]),
    "osh_host_run_liba": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "osh_host_pack_full_inertial": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.POINTER(LibaProblem), c_int64_p, c_int64_p, c_int32_p]),
    "osh_host_run_full_inertial": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_float]),
    "osh_host_get_kf_inertial_gba": (C.c_int64, [C.c_void_p, C.c_int32, c_float_p, c_float_p]),
    "osh_host_pack_merge_inertial": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(LibaProblem), c_int64_p, c_int64_p, c_int32_p, c_int64_p, c_int64_p]),
    "osh_host_run_merge_inertial": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_int64_p, c_double_p]),
    "osh_host_get_kf_velocity": (None, [C.c_void_p, C.c_int32, c_float_p]),
    "osh_host_get_kf_bias": (None, [C.c_void_p, C.c_int32, c_float_p]),
    "osh_host_preintegrate": (C.c_int, [C.c_int32, c_float_p, c_float_p, C.c_float, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]),
    "osh_host_inertial_information": (C.c_int, [c_float_p, c_double_p]),
    "osh_host_frame_create": (C.c_void_p, [C.c_int32, c_float_p, c_int32_p, c_float_p, c_float_p, c_uint8_p, c_float_p, c_float_p,
                                           C.c_float, C.c_float, C.c_int32, C.c_float]),
    "osh_host_frame_set_rig": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_float_p]),
    "osh_host_search_local_points_rig": (C.c_int, [C.c_void_p, C.c_int32, c_uint8_p, c_uint8_p, c_float_p, c_int32_p, c_float_p, c_uint8_p,
                                         c_float_p, c_int32_p, c_float_p, c_int32_p, C.c_float, C.c_float, c_int32_p]),
    "osh_host_frame_set_fisheye": (None, [C.c_void_p, c_float_p]),
    "osh_host_frame_destroy": (None, [C.c_void_p]),
    "osh_host_frame_search_local_points_projected": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_float_p, c_float_p, c_float_p, C.c_float,
                                                              c_uint8_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_uint8_p,
                                                              c_int32_p, C.c_float, C.c_float, c_int32_p, c_int32_p]),
    "osh_host_search_local_points": (C.c_int, [C.c_void_p, C.c_int32, c_uint8_p, c_float_p, c_float_p, c_int32_p, c_float_p, c_float_p,
                                               c_int32_p, C.c_float, C.c_float, c_int32_p]),
    "osh_host_search_last_frame": (C.c_int, [C.c_void_p, C.c_void_p, c_int32_p, C.c_int32, c_float_p, c_uint8_p, C.c_float, C.c_int32,
                                             C.c_int32, c_int32_p]),
    "osh_host_frame_set_camera2": (C.c_int, [C.c_void_p, c_float_p]),
    "osh_host_search_by_bow_kf": (C.c_int, [C.c_int32, c_uint8_p, c_float_p, c_uint8_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p,
                                            C.c_int32, c_uint8_p, c_float_p, c_uint8_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p,
                                            C.c_float, C.c_int32, c_int32_p]),
    "osh_host_search_by_bow": (C.c_int, [C.c_void_p, C.c_int32, c_uint8_p, c_float_p, c_uint8_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p,
                                         C.c_int32, c_int32_p, c_int32_p, c_int32_p, C.c_float, C.c_int32, c_int32_p]),
    "osh_host_frame_pose_optimization": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_int32_p, c_float_p, C.c_int32, c_float_p, c_uint8_p]),
    "osh_host_posei_create": (C.c_void_p, [C.c_int32, C.c_int32, c_float_p, c_int32_p, c_float_p, C.c_int32, c_float_p, c_float_p, c_float_p, c_float_p,
                                           c_float_p, c_float_p, C.c_int32, c_float_p, c_uint8_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                           c_float_p, c_float_p, c_float_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "osh_host_posei_destroy": (None, [C.c_void_p]),
    "osh_host_posei_pack": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PoseiProblem), c_int32_p]),
    "osh_host_posei_run": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_uint8_p, c_double_p, c_int32_p]),
    "osh_host_search_sim3": (C.c_int, [C.c_void_p, c_float_p, C.c_int32, c_float_p, c_uint8_p, c_float_p, c_float_p, c_uint8_p, c_int32_p,
                                       C.c_int32, C.c_float, C.c_int32, c_int32_p, c_int32_p]),
    "osh_host_fuse": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_uint8_p, c_float_p, c_float_p, c_uint8_p, c_uint8_p, c_int32_p, C.c_int32,
                                c_int32_p, c_int32_p, c_uint8_p, C.c_float, c_int32_p, c_uint8_p, c_int32_p, c_int32_p, c_uint8_p, c_int32_p, c_int32_p]),
    "osh_host_fuse_sim3": (C.c_int, [C.c_void_p, c_float_p, C.c_int32, c_float_p, c_uint8_p, c_float_p, c_float_p, c_uint8_p, c_int32_p, c_int32_p,
                                     C.c_int32, c_int32_p, c_uint8_p, C.c_float, c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_search_for_triangulation": (C.c_int, [c_float_p, C.c_int32, C.c_float, C.c_int32, c_float_p, c_int32_p, c_uint8_p, c_uint8_p, c_float_p,
                                                    C.c_int32, c_int32_p, c_int32_p, c_int32_p, C.c_int32, c_float_p, c_int32_p, c_uint8_p, c_uint8_p,
                                                    c_float_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p, C.c_int32, C.c_int32, C.c_int32, c_int32_p]),
    "osh_host_search_for_initialization": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p, C.c_int32, C.c_float, C.c_int32, c_int32_p]),
    "osh_host_pack_gba": (C.c_int, [C.c_void_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_int32_p, c_int32_p, c_uint8_p, c_double_p,
                                    c_double_p, c_int64_p, c_int64_p]),
    "osh_host_pack_welding": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, C.c_int32, c_int32_p, c_int32_p, c_double_p, c_double_p,
                                        c_double_p, c_int32_p, c_int32_p, c_uint8_p, c_double_p, c_double_p, c_int64_p, c_int64_p]),
    "osh_host_run_welding": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, C.c_int32, c_int32_p, c_uint8_p]),
    "osh_host_run_gba": (C.c_int, [C.c_void_p, C.c_int32, c_uint8_p, C.c_int64, C.c_int32]),
    "osh_host_get_kf_pose_gba": (C.c_int64, [C.c_void_p, C.c_int32, c_float_p]),
    "osh_host_get_mp_pos_gba": (C.c_int64, [C.c_void_p, C.c_int32, c_float_p]),
    "osh_host_mp_normal_updates": (C.c_int, [C.c_void_p, C.c_int32]),
    "osh_host_set_bad": (None, [C.c_void_p, C.c_int32, C.c_int32]),
    "osh_host_pack_stereo": (C.c_int, [C.POINTER(HostStereoInput), C.c_int32, c_int32_p, c_float_p, c_int32_p, c_uint8_p, c_float_p, c_int32_p,
                                       c_uint8_p, c_float_p, c_int64_p, c_uint8_p, c_uint8_p, c_float_p]),
    "osh_host_compute_stereo_matches": (C.c_int, [C.POINTER(HostStereoInput), C.c_int32, c_float_p, c_float_p]),
    "osh_host_stereo_restatement": (C.c_int, [C.POINTER(HostStereoInput), c_float_p, c_float_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p,
                                              c_uint8_p, c_uint8_p, c_int32_p, c_double_p]),
    "osh_host_bow_restatement": (C.c_int, [C.POINTER(BowTree), C.c_int32, C.c_int32, c_uint8_p, C.POINTER(BowResult), c_double_p]),
    "osh_host_bow_vocab_load": (C.c_void_p, [C.c_char_p]),
    "osh_host_bow_vocab_free": (None, [C.c_void_p]),
    "osh_host_bow_vocab_tree": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_uint8_p, c_uint8_p, c_double_p, C.c_int32, c_int32_p]),
    "osh_host_bow_compute": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_uint8_p, c_uint8_p, C.c_int32, C.POINTER(BowResult)]),
    "osh_host_bow_score": (C.c_double, [C.c_int32, c_int32_p, c_double_p, C.c_int32, c_int32_p, c_double_p]),
    "osh_host_search_keyframe": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_int32_p, C.c_int32, c_float_p, c_uint8_p, c_float_p,
                                           c_uint8_p, c_uint8_p, c_int32_p, C.c_float, C.c_int32, C.c_int32, c_int32_p]),
}


class HostKfdbGraph(C.Structure):
    """``osh_host_kfdb_graph`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("n_words", C.c_int64), ("n_kf", C.c_int32), ("kf_id", c_int32_p), ("kf_map", c_int32_p), ("kf_bad", c_uint8_p),
                ("bow_start", c_int32_p), ("bow_word", c_int32_p), ("bow_value", c_double_p), ("cov_start", c_int32_p), ("cov", c_int32_p),
                ("con_start", c_int32_p), ("con", c_int32_p), ("n_maps", C.c_int32), ("map_bad", c_uint8_p), ("n_frames", C.c_int32),
                ("fr_id", c_int32_p), ("fr_start", c_int32_p), ("fr_word", c_int32_p), ("fr_value", c_double_p)]


class HostKfdbOut(C.Structure):
    """``osh_host_kfdb_out`` (include/orbslam3_hip_host.h)."""

    _fields_ = [("n_loop", c_int32_p), ("loop", c_int32_p), ("n_merge", c_int32_p), ("merge", c_int32_p), ("marker", c_int64_p),
                ("score", c_float_p)]


(OSH_HOST_KFDB_ADD, OSH_HOST_KFDB_ERASE, OSH_HOST_KFDB_CLEAR_MAP, OSH_HOST_KFDB_CLEAR, OSH_HOST_KFDB_NBEST, OSH_HOST_KFDB_RELOC) = range(6)

_HOST_SIGNATURES.update({
    "osh_host_kfdb_restatement": (C.c_int, [C.POINTER(HostKfdbGraph), C.c_int32, c_int32_p, C.POINTER(HostKfdbOut), c_double_p]),
    "osh_host_kfdb_run": (C.c_int, [C.c_void_p, C.POINTER(HostKfdbGraph), C.c_int32, c_int32_p, C.POINTER(HostKfdbOut), c_double_p]),
    "osh_host_bowdb_check_words": (C.c_int, [C.c_int32, c_int32_p, C.c_int64]),
    "osh_host_bowdb_book_replay": (C.c_int, [C.c_int32, c_int64_p, C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_uint64), c_int64_p, c_int32_p,
                                             c_uint8_p, c_int64_p]),
})


class HostLoop(C.Structure):
    """``osh_host_loop`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("cur", C.c_int32), ("loop", C.c_int32), ("fix_scale", C.c_int32),
        ("n_corrected", C.c_int32), ("corrected_kf", c_int32_p), ("corrected_sim3", c_double_p),
        ("n_noncorrected", C.c_int32), ("noncorrected_kf", c_int32_p), ("noncorrected_sim3", c_double_p),
        ("n_connections", C.c_int32), ("conn_kf", c_int32_p), ("conn_other", c_int32_p),
    ]


class HostMerge(C.Structure):
    """``osh_host_merge`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("cur", C.c_int32), ("n_fixed", C.c_int32), ("fixed", c_int32_p), ("n_fixed_corrected", C.c_int32),
        ("fixed_corrected", c_int32_p), ("n_non_fixed", C.c_int32), ("non_fixed", c_int32_p), ("n_mps", C.c_int32), ("mps", c_int32_p),
    ]


class HostPgoOut(C.Structure):
    """``osh_host_pgo_out`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("max_vertices", C.c_int32), ("max_edges", C.c_int32), ("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("n_free", C.c_int32),
        ("vertex_kf_id", c_int64_p), ("estimate", c_double_p), ("fixed", c_uint8_p), ("fix_scale", c_uint8_p),
        ("edge_ij", c_int32_p), ("measurement", c_double_p),
    ]


class HostPgo4Out(C.Structure):
    """``osh_host_pgo4_out`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("max_vertices", C.c_int32), ("max_edges", C.c_int32), ("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("n_free", C.c_int32),
        ("vertex_kf_id", c_int64_p), ("Rwb", c_double_p), ("twb", c_double_p), ("Rcw", c_double_p), ("tcw", c_double_p),
        ("Rcb", c_double_p), ("tcb", c_double_p), ("fixed", c_uint8_p), ("edge_ij", c_int32_p), ("dR", c_double_p), ("dt", c_double_p),
    ]


_HOST_SIGNATURES.update({
    "osh_host_pgo_set_graph": (C.c_int, [C.c_void_p, c_int32_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p, C.c_int32, c_int32_p, c_int32_p,
                                         c_int32_p, c_uint8_p, c_int32_p, c_int64_p, c_int64_p]),
    "osh_host_pgo_set_before_merge": (None, [C.c_void_p, C.c_int32, c_float_p]),
    "osh_host_pgo_pack": (C.c_int, [C.c_void_p, C.POINTER(HostLoop), C.POINTER(HostPgoOut)]),
    "osh_host_pgo_pack_merge": (C.c_int, [C.c_void_p, C.POINTER(HostMerge), C.POINTER(HostPgoOut)]),
    "osh_host_pgo_run": (C.c_int, [C.c_void_p, C.POINTER(HostLoop)]),
    "osh_host_pgo_run_merge": (C.c_int, [C.c_void_p, C.POINTER(HostMerge)]),
    "osh_host_sim3_apply": (C.c_int, [C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p, c_uint8_p, c_double_p]),
    "osh_host_pgo4_pack": (C.c_int, [C.c_void_p, C.POINTER(HostLoop), C.POINTER(HostPgo4Out)]),
    "osh_host_pgo4_run": (C.c_int, [C.c_void_p, C.POINTER(HostLoop)]),
    "osh_host_pgo4_apply": (C.c_int, [C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p]),
    "osh_host_pgo4_sizes": (None, [c_int64_p]),
})
class HostSim3Kf(C.Structure):
    """``osh_host_sim3_kf`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("pose", C.c_float * 7), ("cam", C.c_float * 8), ("kb8", C.c_int32), ("n_keys", C.c_int32), ("keys_un", c_float_p),
        ("octave", c_int32_p), ("n_levels", C.c_int32), ("inv_level_sigma2", c_float_p),
    ]


class HostSim3Input(C.Structure):
    """``osh_host_sim3_input`` (include/orbslam3_hip_host.h)."""

    _fields_ = [
        ("kf1", HostSim3Kf), ("kf2", HostSim3Kf), ("n_points", C.c_int32), ("mp_pos", c_float_p), ("mp_bad", c_uint8_p),
        ("mp_index2", c_int32_p), ("mp_track_level", c_int32_p), ("kf1_mp", c_int32_p), ("n_matches", C.c_int32),
        ("matches1", c_int32_p), ("S12", C.c_double * 8), ("th2", C.c_float), ("fix_scale", C.c_int32), ("all_points", C.c_int32),
    ]


_HOST_SIGNATURES.update({
    "osh_host_pack_sim3": (C.c_int, [C.POINTER(HostSim3Input), C.c_int32, C.POINTER(Sim3Problem), c_int32_p] + [c_double_p] * 6),
    "osh_host_optimize_sim3": (C.c_int, [C.POINTER(HostSim3Input), c_uint8_p, c_double_p, c_double_p]),
})

# MapPoint::RefreshBatch, LocalMapping::SearchInNeighbors / ProcessNewKeyFrame (csrc/hosttest/mappoints.cc)
_HOST_SIGNATURES.update({
    "osh_host_mappoint_refresh_cpu": (C.c_int, [C.c_int32, C.POINTER(MapPointBatch), C.POINTER(MapPointResult), c_double_p]),
    "osh_host_graph_set_mapping": (C.c_int, [C.c_void_p, C.c_float, C.c_int32, c_float_p, C.c_float, c_int32_p, c_uint8_p]),
    "osh_host_graph_set_ref_kf": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p]),
    "osh_host_graph_unlink": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "osh_host_graph_clone_point": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, c_int32_p]),
    "osh_host_mp_refresh_batch": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p]),
    "osh_host_mp_refresh_pack": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_uint8_p,
                                           c_int32_p, c_uint8_p, c_float_p, c_float_p, c_int32_p, c_float_p, c_float_p]),
    "osh_host_mp_get_refresh": (C.c_int, [C.c_void_p, C.c_int32, c_uint8_p, c_float_p, c_float_p, c_int32_p]),
    "osh_host_mp_observations": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_mp_state": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p]),
    "osh_host_kf_matches": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p]),
    "osh_host_kf_state": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p, c_float_p]),
    "osh_host_graph_fuse": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, C.c_float, C.c_int32]),
    "osh_host_local_mapping_search_in_neighbors": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "osh_host_local_mapping_process_new_keyframe": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
})

# LocalMapping::KeyFrameCulling / MapPointCulling and their stand-in map (csrc/hosttest/kfcull.cc)
_HOST_SIGNATURES.update({
    "osh_host_cull_graph_create": (C.c_void_p, [C.POINTER(HostCullScene)]),
    "osh_host_local_mapping_keyframe_culling": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
    "osh_host_local_mapping_map_point_culling": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_int32_p, C.c_int32, c_int32_p]),
    "osh_host_mp_set_culling": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "osh_host_kfcull_pack": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p,
                                       c_int32_p, c_int32_p, c_int32_p, c_uint8_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_keyframe_cull_cpu": (C.c_int, [C.POINTER(KfCullProblem), C.c_int32, c_int32_p, C.c_int32, C.POINTER(KfCullResult), c_double_p]),
    "osh_host_kfcull_time": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.c_int32, c_double_p, c_int64_p]),
    "osh_host_kf_cull_state": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p]),
    "osh_host_mp_cull_state": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p]),
})

# ORBmatcher::Fuse for many targets (csrc/hosttest/fuse_batch.cc)
_HOST_SIGNATURES.update({
    "osh_host_fuse_search_cpu": (C.c_int, [C.c_int32, C.POINTER(FuseTarget), C.POINTER(FusePoints), C.c_int32, C.POINTER(FuseResult), c_double_p]),
    "osh_host_set_recompute_descriptors": (None, [C.c_int32]),
    "osh_host_graph_fuse_batch": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, c_uint8_p, C.c_int32, c_int32_p, C.c_int32, c_int32_p, c_int32_p]),
    "osh_host_graph_fuse_batch_sim3": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.c_int32, c_int32_p, C.c_float, C.c_int32, C.c_int32,
                                                 c_int32_p, c_int32_p, c_int32_p]),
    "osh_host_graph_fuse_sim3": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, C.c_int32, c_int32_p, C.c_float, c_int32_p]),
    "osh_host_graph_replace": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "osh_host_graph_fuse_candidates": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, C.c_float, C.c_int32, C.c_int32, c_int32_p, c_int32_p, C.c_int32, c_int32_p]),
    "osh_host_graph_fuse_pack_search": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, C.c_float, C.c_int32, C.c_int32, c_int32_p, C.c_int32] + [c_int32_p] * 4),
    "osh_host_loop_search_and_fuse": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, c_double_p, C.c_int32, c_int32_p, C.c_int32, c_int32_p, c_int32_p]),
})


HOST_EXPORTED_SYMBOLS = tuple(_HOST_SIGNATURES)

# osh_host_pgo4_apply operations (include/orbslam3_hip_host.h)
OSH_PGO4_EXP, OSH_PGO4_LOG, OSH_PGO4_NORMALIZE, OSH_PGO4_UPDATE, OSH_PGO4_EDGE_ERROR = range(5)

_lib = None
_host_lib = None


def _open(p: Path, signatures: dict) -> C.CDLL:
    if not p.exists():
        raise RuntimeError(
            f"{p} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the product path)."
        )
    lib = C.CDLL(str(p))
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """Load liborbslam3_hip.so (built by ``__graft_entry__.build()``); raise if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # ORBSLAM3_HIP_LIB: developer aid for A/B runs of an alternative build of the same library
    lib = _open(Path(path) if path else Path(os.environ.get("ORBSLAM3_HIP_LIB", LIB_PATH)), _SIGNATURES)
    if path is None:
        _lib = lib
    return lib


def load_host_library() -> C.CDLL:
    """Load liborbslam3_hip_hosttest.so (the C++ host layer and its test wrappers); raise if absent.

    The kernel library is loaded first: it carries the soname the host library depends on, so an ORBSLAM3_HIP_LIB
    override also serves the host library and the process holds one copy of it (one osh_last_error text)."""
    global _host_lib
    if _host_lib is None:
        load_library()
        _host_lib = _open(HOST_LIB_PATH, _HOST_SIGNATURES)
    return _host_lib


def last_error(lib=None) -> str:
    lib = lib or load_library()
    s = lib.osh_last_error()
    return s.decode() if s else ""


class OshError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where} failed with code {code}: {msg}")
        self.code = code


def check(code: int, where: str, lib=None):
    if code != OSH_OK:
        raise OshError(code, where, last_error(lib))


def np_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)
