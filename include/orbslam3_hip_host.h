/*
 * orbslam3_hip_host.h -- C entry points of the C++ host layer (csrc/host/), for tests and bindings.  Defined in
 * csrc/hosttest/harness.cc and exported by the test-only liborbslam3_hip_hosttest.so, not by liborbslam3_hip.so.
 *
 * The drop-in itself is C++: ORB_SLAM3::Optimizer::LocalBundleAdjustment (include/Optimizer.h) and
 * ORB_SLAM3::ORBmatcher::SearchByProjection (include/ORBmatcher.h), same signatures as the reference.
 * These C wrappers build a KeyFrame / MapPoint / Map (or Frame) graph from flat arrays, call the C++
 * entry points and read the graph back, so the boundary can be exercised from ctypes.
 */
#ifndef ORBSLAM3_HIP_HOST_H
#define ORBSLAM3_HIP_HOST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct osh_host_graph osh_host_graph;

/* Wall time (ms) of the product call (Optimizer:: / ORBmatcher:: entry point) inside the last harness wrapper on this thread,
 * without the construction of the KeyFrame / MapPoint / Frame objects around it. */
double osh_host_last_call_ms(void);

/* Build a map: n_kf keyframes (ids kf_id, poses Tcw as qx qy qz qw tx ty tz floats, one shared pinhole
 * fx fy cx cy + bf), n_mp map points, n_obs observations (keyframe index, point index, u v ur with ur<0 for
 * monocular, octave).  Keypoint k of a keyframe is its k-th observation in array order. */
osh_host_graph* osh_host_graph_create(int32_t n_kf, const int64_t* kf_id, const float* kf_pose_qt, const float* cam5,
                                      const float* inv_level_sigma2, int32_t n_levels,
                                      int32_t n_mp, const int64_t* mp_id, const float* mp_pos,
                                      int32_t n_obs, const int32_t* obs_kf, const int32_t* obs_mp, const float* obs_uvr,
                                      const int32_t* obs_octave, int64_t init_kf_id, int32_t inertial);
/* Turn the map into a fisheye STEREO rig (call after osh_host_graph_set_fisheye): right camera cam2 = fx fy cx cy k1..k4,
 * Trl = qx qy qz qw tx ty tz, and n_obs right-camera observations (keyframe index, map point index, u v, octave) which become
 * mvKeysRight entries observed through the right slot of MapPoint::GetObservations()'s tuples. */
int osh_host_graph_set_rig(osh_host_graph* g, const float cam2[8], const float trl_qt[7], int32_t n_obs, const int32_t* obs_kf,
                           const int32_t* obs_mp, const float* obs_uv, const int32_t* obs_octave);
void osh_host_graph_destroy(osh_host_graph* g);
/* Camera model of the window the last osh_host_pack_lba / _gba / _welding call built: 1 + k1..k4 for KannalaBrandt8, else 0. */
int osh_host_last_pack_kb8(osh_host_graph* g, double k[4]);
/* Same for the rig description of a fisheye stereo window: returns 1 and fills cam2[8] / trl[7], else 0. */
int osh_host_last_pack_rig(osh_host_graph* g, double cam2[8], double trl[7]);
/* Switch the map's camera to a KannalaBrandt8 (same fx fy cx cy, coefficients k1..k4): a monocular fisheye map. */
void osh_host_graph_set_fisheye(osh_host_graph* g, const float k[4]);
/* covisibility list returned by KeyFrame::GetVectorCovisibleKeyFrames() of keyframe kf_index */
int osh_host_graph_set_covisible(osh_host_graph* g, int32_t kf_index, int32_t n, const int32_t* kf_indices);

/* Steps 1-6 of Optimizer::LocalBundleAdjustment only (graph -> osh_lba_problem arrays); no GPU needed.
 * sizes = {P, F, L, E, num_fixedKF}; every array may be NULL.  Returns 0, 1 (no fixed keyframe) or <0. */
int osh_host_pack_lba(osh_host_graph* g, int32_t kf_index, int32_t sizes[5], double* pose_qt, double* pose_cam,
                      double* points, int32_t* edge_pose, int32_t* edge_point, uint8_t* edge_kind, double* edge_obs,
                      double* edge_info, int64_t* pose_kf_id, int64_t* point_mp_id);
/* ORB_SLAM3::Optimizer::LocalBundleAdjustment(kf, stop_flag, map, ...); counts = num_fixedKF, num_OptKF, num_MPs, num_edges */
int osh_host_run_lba(osh_host_graph* g, int32_t kf_index, unsigned char* stop_flag, int32_t counts[4]);

void osh_host_get_kf_pose(osh_host_graph* g, int32_t kf_index, float out_qt[7]);
void osh_host_get_mp_pos(osh_host_graph* g, int32_t mp_index, float out[3]);
int  osh_host_mp_num_observations(osh_host_graph* g, int32_t mp_index);   /* size of GetObservations() */
int  osh_host_mp_is_bad(osh_host_graph* g, int32_t mp_index);
int  osh_host_kf_num_matches(osh_host_graph* g, int32_t kf_index);        /* non-null GetMapPointMatches() */
int  osh_host_kf_observes(osh_host_graph* g, int32_t kf_index, int32_t mp_index);
int  osh_host_map_change_index(osh_host_graph* g);
int  osh_host_kf_pose_sets(osh_host_graph* g, int32_t kf_index);

/* ---- inertial ---- */
/* Attach IMU state to the first n keyframes listed: previous keyframe (index or -1), velocity, bias (bax bay baz bwx bwy bwz),
 * the preintegration from the previous keyframe (OSH_PREINT_FLOATS record, dT == 0: none) with its 15x15 covariance, and the
 * camera-IMU calibration T_bc (qx qy qz qw tx ty tz).  Every keyframe of the map gets the calibration. */
int osh_host_graph_set_inertial(osh_host_graph* g, int32_t n, const int32_t* kf_index, const int32_t* prev_index, const float* vel,
                                const float* bias6, const float* preint, const float* cov225, const float* Tbc_qt);
/* Window selection + packing of Optimizer::LocalInertialBA (no GPU): fills *out with pointers into storage owned by the
 * graph (valid until the next call).  pose_kf_id / point_mp_id (may be NULL) receive the ids in problem order. */
struct osh_liba_problem;
int osh_host_pack_liba(osh_host_graph* g, int32_t kf_index, int32_t b_large, int32_t b_rec_init, struct osh_liba_problem* out,
                       int64_t* pose_kf_id, int64_t* point_mp_id);
/* ORB_SLAM3::Optimizer::LocalInertialBA(kf, NULL, map, ..., bLarge, bRecInit) */
int osh_host_run_liba(osh_host_graph* g, int32_t kf_index, int32_t b_large, int32_t b_rec_init);
/* Optimizer::FullInertialBA(&map, its, bFixLocal, nLoopId, NULL, bInit) (src/Optimizer.cc:393-814): the flat problem it solves
 * (pack; *n_idle = keyframes no edge touches) and the call itself.  -3: a case the device path does not take (message on stderr). */
int osh_host_pack_full_inertial(osh_host_graph* g, int32_t its, int32_t fix_local, int32_t b_init, float prior_g, float prior_a,
                                struct osh_liba_problem* out, int64_t* pose_kf_id, int64_t* point_mp_id, int32_t* n_idle);
int osh_host_run_full_inertial(osh_host_graph* g, int32_t its, int32_t fix_local, int64_t loop_id, int32_t b_init, float prior_g, float prior_a);
int64_t osh_host_get_kf_inertial_gba(osh_host_graph* g, int32_t i, float vel[3], float bias6[6]);   /* mVwbGBA, mBiasGBA; returns mnBAGlobalForKF */
/* Optimizer::MergeInertialBA(curr, merge, NULL, &map, corrPoses) (src/Optimizer.cc:3956-4498).  n_sets = {temporal, covisible}
 * keyframe counts with their ids in the reference's order; run returns corrPoses.size() and copies {id; qx qy qz qw tx ty tz s}. */
int osh_host_pack_merge_inertial(osh_host_graph* g, int32_t curr, int32_t merge, struct osh_liba_problem* out, int64_t* pose_kf_id,
                                 int64_t* point_mp_id, int32_t n_sets[2], int64_t* temporal_kf_id, int64_t* cov_kf_id);
int osh_host_run_merge_inertial(osh_host_graph* g, int32_t curr, int32_t merge, int32_t max_corr, int64_t* corr_kf_id, double* corr_sim3);
void osh_host_get_kf_velocity(osh_host_graph* g, int32_t kf_index, float out[3]);
void osh_host_get_kf_bias(osh_host_graph* g, int32_t kf_index, float out6[6]);
/* IMU::Preintegrated: integrate n measurements (float32 recursion) -> record + covariance */
int osh_host_preintegrate(int32_t n, const float* acc, const float* gyr, float dt, const float* bias6, const float* nga6,
                          const float* walk6, float* rec_out, float* cov225_out);
/* EdgeInertial information from a 15x15 preintegration covariance (inverse, symmetrise, eigenvalue clamp) */
int osh_host_inertial_information(const float* cov225, double* info81_out);

/* ---- matcher ---- */
/* Optimizer::GlobalBundleAdjustemnt(&map, n_iterations, stop_flag, n_loop_kf, robust) on every keyframe and point of the graph
 * (src/Optimizer.cc:53-392).  pack: the osh_lba_problem the host layer builds (sizes = {n_free, n_fixed, n_points, n_edges,
 * points without any edge}); the GBA getters return mnBAGlobalForKF and fill mTcwGBA / mPosGBA. */
int osh_host_pack_gba(osh_host_graph* g, int32_t sizes[5], double* pose_qt, double* pose_cam, double* points,
                      int32_t* edge_pose, int32_t* edge_point, uint8_t* edge_kind, double* edge_obs, double* edge_info,
                      int64_t* pose_kf_id, int64_t* point_mp_id);
/* The welding Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) (src/Optimizer.cc:3506-3955); pack =
 * the problem of its first optimisation. */
int osh_host_pack_welding(osh_host_graph* g, int32_t main_index, int32_t n_adj, const int32_t* adj, int32_t n_fix,
                          const int32_t* fix, int32_t sizes[5], double* pose_qt, double* pose_cam, double* points,
                          int32_t* edge_pose, int32_t* edge_point, uint8_t* edge_kind, double* edge_obs, double* edge_info,
                          int64_t* pose_kf_id, int64_t* point_mp_id);
int osh_host_run_welding(osh_host_graph* g, int32_t main_index, int32_t n_adj, const int32_t* adj, int32_t n_fix,
                         const int32_t* fix, unsigned char* stop_flag);
int osh_host_run_gba(osh_host_graph* g, int32_t n_iterations, unsigned char* stop_flag, int64_t n_loop_kf, int32_t robust);
int64_t osh_host_get_kf_pose_gba(osh_host_graph* g, int32_t kf_index, float pose_qt[7]);
int64_t osh_host_get_mp_pos_gba(osh_host_graph* g, int32_t mp_index, float pos[3]);
int osh_host_mp_normal_updates(osh_host_graph* g, int32_t mp_index);
void osh_host_set_bad(osh_host_graph* g, int32_t kf_index, int32_t mp_index);   /* marks a keyframe and/or a point bad (-1: none) */

typedef struct osh_host_frame osh_host_frame;
/* A frame with n keypoints (x y, octave, angle, uRight (<=0: none), 32-byte descriptor), pose Tcw. */
osh_host_frame* osh_host_frame_create(int32_t n, const float* kp_xy, const int32_t* octave, const float* angle,
                                      const float* uright, const uint8_t* desc, const float pose_qt[7],
                                      const float cam4[4], float mbf, float mb, int32_t n_levels, float scale_factor);
/* Fisheye STEREO frame: the first n_left keypoints become the left camera's, the rest the right camera's (descriptor rows
 * [n_left, N)); left_to_right[n_left] / right_to_left[N - n_left] are Frame::mvLeftToRightMatch / mvRightToLeftMatch. */
int osh_host_frame_set_rig(osh_host_frame* f, int32_t n_left, const int32_t* left_to_right, const int32_t* right_to_left, const float trl_qt[7]);
/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) on such a frame (src/ORBmatcher.cc:43-213, both camera
 * passes); per map point the tracking fields of both cameras; assignment[N] = map point stored in each keypoint slot or -1. */
int osh_host_search_local_points_rig(osh_host_frame* f, int32_t n_mp, const uint8_t* mp_desc, const uint8_t* in_left,
                                     const float* proj_left, const int32_t* level_left, const float* viewcos_left,
                                     const uint8_t* in_right, const float* proj_right, const int32_t* level_right,
                                     const float* viewcos_right, const int32_t* n_observations, float nnratio, float th,
                                     int32_t* assignment);
int osh_host_frame_set_camera2(osh_host_frame* f, const float cam2[8]);
int osh_host_search_by_bow_kf(int32_t n1, const uint8_t* desc1, const float* angle1, const uint8_t* has_mp1, int32_t nodes1,
                              const int32_t* node_id1, const int32_t* node_off1, const int32_t* node_feat1, int32_t n2,
                              const uint8_t* desc2, const float* angle2, const uint8_t* has_mp2, int32_t nodes2, const int32_t* node_id2,
                              const int32_t* node_off2, const int32_t* node_feat2, float nnratio, int32_t check_ori, int32_t* match12);
int osh_host_search_by_bow(osh_host_frame* f, int32_t n_kf, const uint8_t* kf_desc, const float* kf_angle, const uint8_t* kf_has_mp,
                           int32_t kf_nodes, const int32_t* kf_node_id, const int32_t* kf_node_off, const int32_t* kf_node_feat,
                           int32_t f_nodes, const int32_t* f_node_id, const int32_t* f_node_off, const int32_t* f_node_feat,
                           float nnratio, int32_t check_ori, int32_t* assignment);
void osh_host_frame_destroy(osh_host_frame* f);
/* Switch the frame's camera to a KannalaBrandt8 (same fx fy cx cy, coefficients k1..k4). */
void osh_host_frame_set_fisheye(osh_host_frame* f, const float k[4]);
/* ORBmatcher(nnratio).SearchByProjection(F, vpMapPoints, th): map points given by their tracking scratch
 * (mTrackProjX/Y/XR, mnTrackScaleLevel, mTrackViewCos, mTrackDepth), descriptor and Observations().
 * assignment[k] = index of the map point stored in F.mvpMapPoints[k] or -1.  Returns nmatches (<0: error). */
int osh_host_search_local_points(osh_host_frame* f, int32_t n_mp, const uint8_t* mp_desc, const float* proj_xy,
                                 const float* proj_xr, const int32_t* level, const float* viewcos, const float* depth,
                                 const int32_t* n_observations, float nnratio, float th, int32_t* assignment);
/* Frame::isInFrustum(pMP, viewing_cos_limit) for every map point (the loop of Tracking::SearchLocalPoints,
 * src/Tracking.cc:3411-3432) as one device launch; outputs are the MapPoint tracking fields afterwards.  With
 * assignment != NULL it continues with ORBmatcher(nnratio).SearchByProjection(F, vpMapPoints, th) (:3460) like
 * osh_host_search_local_points.  Returns the number of points in view (<0: error). */
int osh_host_frame_search_local_points_projected(osh_host_frame* f, int32_t n_mp, const float* mp_pos, const float* mp_normal,
                                                 const float* mp_min_dist, const float* mp_max_dist, float viewing_cos_limit,
                                                 uint8_t* in_view, float* proj_xy, float* proj_xr, float* depth, float* view_cos,
                                                 int32_t* level, const uint8_t* mp_desc, const int32_t* n_observations,
                                                 float nnratio, float th, int32_t* assignment, int32_t* n_matches);
/* ORBmatcher(nnratio, check_ori).SearchByProjection(Current, Last, th, bMono): last_mp[k] = map point index held by
 * keypoint k of the last frame (-1 none); map points given by world position + descriptor. */
int osh_host_search_last_frame(osh_host_frame* cur, osh_host_frame* last, const int32_t* last_mp, int32_t n_mp,
                               const float* mp_pos, const uint8_t* mp_desc, float th, int32_t b_mono, int32_t check_ori,
                               int32_t* assignment);
/* ORBmatcher(0.9, check_ori).SearchByProjection(Current, pKF, sAlreadyFound, th, ORBdist) (relocalisation,
 * src/ORBmatcher.cc:1889-2010): the keyframe is given by its keypoint angles and kf_mp[k] = map point held by keypoint k
 * (-1 none); map points by world position, descriptor, {mfMinDistance, mfMaxDistance}, membership of sAlreadyFound, isBad();
 * cur_mp[k] = map point already held by keypoint k of the current frame (-1 none). */
int osh_host_search_keyframe(osh_host_frame* cur, int32_t n_kf, const float* kf_angle, const int32_t* kf_mp, int32_t n_mp,
                             const float* mp_pos, const uint8_t* mp_desc, const float* mp_min_max_dist,
                             const uint8_t* mp_found, const uint8_t* mp_bad, const int32_t* cur_mp, float th,
                             int32_t orb_dist, int32_t check_ori, int32_t* assignment);
/* ORBmatcher::SearchByProjection(KeyFrame*, Sim3f&, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming)
 * (src/ORBmatcher.cc:427-646): the keyframe is made from `f`; scw = unit quaternion (x y z w), translation, scale;
 * map points by world position, descriptor, {mfMinDistance, mfMaxDistance}, normal, isBad(); matched_in[k] = map point
 * already matched to keypoint k (-1 none).  with_keyframes selects the second overload (point j comes from keyframe j). */
int osh_host_search_sim3(osh_host_frame* f, const float scw[8], int32_t n_mp, const float* mp_pos, const uint8_t* mp_desc,
                         const float* mp_min_max_dist, const float* mp_normal, const uint8_t* mp_bad,
                         const int32_t* matched_in, int32_t th, float ratio_hamming, int32_t with_keyframes,
                         int32_t* matched_out, int32_t* matched_kf_out);
/* ORBmatcher(nnratio, check_ori).SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:648-763):
 * prev_xy[n1][2] is vbPrevMatched (updated in place), matches12[n1] = vnMatches12. */
int osh_host_search_for_initialization(osh_host_frame* f1, osh_host_frame* f2, float* prev_xy, int32_t window, float nnratio, int32_t check_ori,
                                       int32_t* matches12);
/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:907-1146) on two pinhole
 * keyframes: kp[n][4] = x, y, angle, uright (< 0: monocular), vocabulary nodes as (id, offsets, features), poses as unit quaternion
 * (x y z w) + translation of Tcw.  match12[i] = feature of keyframe 2 paired with feature i of keyframe 1 (-1 none). */
int osh_host_search_for_triangulation(const float cam4[4], int32_t n_levels, float scale_factor, int32_t n1, const float* kp1,
                                      const int32_t* octave1, const uint8_t* desc1, const uint8_t* has_mp1, const float pose1_qt[7],
                                      int32_t nodes1, const int32_t* node_id1, const int32_t* node_off1, const int32_t* node_feat1,
                                      int32_t n2, const float* kp2, const int32_t* octave2, const uint8_t* desc2, const uint8_t* has_mp2,
                                      const float pose2_qt[7], int32_t nodes2, const int32_t* node_id2, const int32_t* node_off2,
                                      const int32_t* node_feat2, int32_t only_stereo, int32_t coarse, int32_t check_ori, int32_t* match12);
/* ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:1148-1338): the keyframe is made from `f` (its pose,
 * keypoints, grid, mvuRight).  Candidate map points j (null_mask[j]: a null entry) with world position, descriptor, {mfMinDistance,
 * mfMaxDistance}, normal, isBad(), Observations(); resident map points r already sitting in keypoint slots (slot_res[k] = r or -1).
 * Ids in the outputs: candidate j -> j, resident r -> 100000 + r, none -> -1.  slot_out[k]: the keyframe's match at keypoint k
 * afterwards; *_replaced_out: GetReplaced(); *_nobs_out: Observations() afterwards.  Returns nFused. */
int osh_host_fuse(osh_host_frame* f, int32_t n_mp, const float* mp_pos, const uint8_t* mp_desc, const float* mp_min_max_dist,
                  const float* mp_normal, const uint8_t* mp_bad, const uint8_t* null_mask, const int32_t* mp_nobs,
                  int32_t n_res, const int32_t* slot_res, const int32_t* res_nobs, const uint8_t* res_bad, float th,
                  int32_t* slot_out, uint8_t* cand_bad_out, int32_t* cand_replaced_out, int32_t* cand_nobs_out,
                  uint8_t* res_bad_out, int32_t* res_replaced_out, int32_t* res_nobs_out);
/* ORBmatcher::Fuse(KeyFrame*, Sim3f&, const vector<MapPoint*>&, th, vpReplacePoint) (src/ORBmatcher.cc:1340-1455): as osh_host_fuse;
 * found_slot[j] >= 0: candidate j already sits in the keyframe at that keypoint (spAlreadyFound); replace_out[j]: id of
 * vpReplacePoint[j] (-1 null). */
int osh_host_fuse_sim3(osh_host_frame* f, const float scw[8], int32_t n_mp, const float* mp_pos, const uint8_t* mp_desc,
                       const float* mp_min_max_dist, const float* mp_normal, const uint8_t* mp_bad, const int32_t* mp_nobs,
                       const int32_t* found_slot, int32_t n_res, const int32_t* slot_res, const uint8_t* res_bad, float th,
                       int32_t* slot_out, int32_t* replace_out, int32_t* cand_nobs_out);
/* Optimizer::PoseOptimization(&frame) (src/Optimizer.cc:815-1114): kp_mp[k] = map point matched to keypoint k (-1 none);
 * returns the inlier count, the optimised pose and mvbOutlier (keypoints without a match keep the value 1 they are preset to). */
int osh_host_frame_pose_optimization(osh_host_frame* f, int32_t n_mp, const float* mp_pos, const int32_t* kp_mp,
                                     const float* inv_level_sigma2, int32_t n_levels, float pose_out[7], uint8_t* outlier_out);
/* ---- Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame on a test frame (csrc/hosttest/harness.cc) */
typedef struct osh_host_posei osh_host_posei;
osh_host_posei* osh_host_posei_create(int32_t mode, int32_t n_kp, const float* kp_xy, const int32_t* octave, const float* uright,
                                      int32_t n_left, const float pose_qt[7], const float cam5[5], const float* kb8,
                                      const float* cam2_8, const float* trl_qt, const float* inv_level_sigma2, int32_t n_levels,
                                      const float* mp_pos, const uint8_t* mp_close, const float Tbc_qt[7], const float vel[3],
                                      const float bias6[6], const float prev_pose_qt[7], const float prev_vel[3], const float prev_bias6[6],
                                      const float* preint72, const float* cov225, const double* prior_Rwb, const double* prior_twb,
                                      const double* prior_vel, const double* prior_bg, const double* prior_ba, const double* prior_H);
void osh_host_posei_destroy(osh_host_posei* h);
int osh_host_posei_pack(osh_host_posei* h, int32_t rec_init, osh_posei_problem* out, int32_t* kp_of_edge);
int osh_host_posei_run(osh_host_posei* h, int32_t rec_init, float pose_out[7], float Rwb_out[9], float twb_out[3], float vel_out[3],
                       float bias6_out[6], uint8_t* outlier_out, double* H225_out, int32_t* prev_cpi_deleted);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (src/ORBmatcher.cc:1457-1674), two frames standing in for the keyframes.
 * slot_mp_k[i]: index of the map point in keypoint slot i of keyframe k (into its own point list) or -1; matches_in[i1]: keyframe-2
 * point already matched to slot i1 or -1; matches_out[i1]: keyframe-2 point index or -1.  s12 = qx qy qz qw tx ty tz s. */
int osh_host_search_by_sim3(osh_host_frame* f1, osh_host_frame* f2, const float s12[8], float th,
                            int32_t n_mp1, const float* mp_pos1, const uint8_t* mp_desc1, const float* mp_min_max1, const uint8_t* mp_bad1,
                            const int32_t* slot_mp1, int32_t n_mp2, const float* mp_pos2, const uint8_t* mp_desc2, const float* mp_min_max2,
                            const uint8_t* mp_bad2, const int32_t* slot_mp2, const int32_t* matches_in, int32_t* matches_out);

/* ---- Optimizer::OptimizeEssentialGraph (csrc/host/OptimizerEssentialGraph.cc) on a map made by osh_host_graph_create ---- */
/* The essential graph of the stand-in map: parent[n_kf] (keyframe index, -1: none; children follow), covisibility entries
 * (keyframe, other keyframe, weight; each keyframe's list is ordered by descending weight, ties in entry order), loop edges
 * (both directions), prev_kf[n_kf] / b_imu[n_kf] (may be NULL), and per map point its reference keyframe index, mnCorrectedByKF
 * and mnCorrectedReference (may be NULL). */
int osh_host_pgo_set_graph(osh_host_graph* g, const int32_t* parent, int32_t n_cov, const int32_t* cov_kf, const int32_t* cov_other,
                           const int32_t* cov_weight, int32_t n_loop, const int32_t* loop_a, const int32_t* loop_b, const int32_t* prev_kf,
                           const uint8_t* b_imu, const int32_t* mp_ref, const int64_t* mp_corrected_by, const int64_t* mp_corrected_ref);
/* mTcwBefMerge (and mTwcBefMerge, its inverse) of keyframe kf_index: qx qy qz qw tx ty tz */
void osh_host_pgo_set_before_merge(osh_host_graph* g, int32_t kf_index, const float qt[7]);
/* The loop correction handed to the first overload (keyframes by index; Sim3 as qx qy qz qw tx ty tz s). */
typedef struct osh_host_loop {
  int32_t cur, loop, fix_scale;
  int32_t n_corrected;    const int32_t* corrected_kf;    const double* corrected_sim3;      /* CorrectedSim3    */
  int32_t n_noncorrected; const int32_t* noncorrected_kf; const double* noncorrected_sim3;   /* NonCorrectedSim3 */
  int32_t n_connections;  const int32_t* conn_kf;         const int32_t* conn_other;         /* LoopConnections  */
} osh_host_loop;
/* The three keyframe lists and the map points of the merge overload (indices). */
typedef struct osh_host_merge {
  int32_t cur;
  int32_t n_fixed;           const int32_t* fixed;
  int32_t n_fixed_corrected; const int32_t* fixed_corrected;
  int32_t n_non_fixed;       const int32_t* non_fixed;
  int32_t n_mps;             const int32_t* mps;
} osh_host_merge;
/* What the graph walk built: capacities in, sizes out; arrays as osh_pgo_problem, vertex_kf_id = mnId of every vertex. */
typedef struct osh_host_pgo_out {
  int32_t max_vertices, max_edges;
  int32_t n_vertices, n_edges, n_free;
  int64_t* vertex_kf_id; double* estimate; uint8_t* fixed; uint8_t* fix_scale; int32_t* edge_ij; double* measurement;
} osh_host_pgo_out;
/* The graph walk alone (no device): 0, or -1 when a capacity is too small. */
int osh_host_pgo_pack(osh_host_graph* g, const osh_host_loop* loop, osh_host_pgo_out* out);
int osh_host_pgo_pack_merge(osh_host_graph* g, const osh_host_merge* merge, osh_host_pgo_out* out);
/* ORB_SLAM3::Optimizer::OptimizeEssentialGraph, either overload */
int osh_host_pgo_run(osh_host_graph* g, const osh_host_loop* loop);
int osh_host_pgo_run_merge(osh_host_graph* g, const osh_host_merge* merge);
/* Optimizer::OptimizeEssentialGraph4DoF (csrc/host/OptimizerEssentialGraph4DoF.cc) on the same stand-in map: the graph from
 * osh_host_pgo_set_graph (prev_kf also sets mNextKF), mImuCalib from osh_host_graph_set_inertial.  osh_host_loop's fix_scale is
 * not read.  The walk alone (0, or -1 when a capacity is too small; arrays as osh_pgo4_problem) and the call itself. */
typedef struct osh_host_pgo4_out {
  int32_t max_vertices, max_edges;
  int32_t n_vertices, n_edges, n_free;
  int64_t* vertex_kf_id; double* Rwb; double* twb; double* Rcw; double* tcw; double* Rcb; double* tcb; uint8_t* fixed;
  int32_t* edge_ij; double* dR; double* dt;
} osh_host_pgo4_out;
int osh_host_pgo4_pack(osh_host_graph* g, const osh_host_loop* loop, osh_host_pgo4_out* out);
int osh_host_pgo4_run(osh_host_graph* g, const osh_host_loop* loop);
/* UpdateNormalAndDepth calls on map point mp_index (osh_host_mp_normal_updates) and pose writes (osh_host_kf_pose_sets) count the
 * write-back; osh_host_map_change_index counts IncreaseChangeIndex. */

/* ---- the device's Sim3 algebra (csrc/pgo_sim3.h) compiled for the host ---- */
/* op over n items, Sim3 = qx qy qz qw tx ty tz s (8 doubles), tangent = omega upsilon sigma (7), R row-major (9):
 *   EXP a[7] -> out[8]          LOG a[8] -> out[7]          MUL a[8] b[8] -> out[8]      INVERSE a[8] -> out[8]
 *   MAP a[8] b[3] -> out[3]     EDGE_ERROR meas a[8], Si b[8], Sj c[8] -> out[7]     OPLUS est a[8], update b[7], flag = fix_scale -> out[8]
 *   QUAT_TO_R a[4] -> out[9]    R_TO_QUAT a[9] -> out[4]    SOLVE3 (3x3 partial-pivot LU) W a[9] t b[3] -> out[3]
 * Returns 0, or -1 for an unknown op or a missing array. */
#define OSH_SIM3_EXP        0
#define OSH_SIM3_LOG        1
#define OSH_SIM3_MUL        2
#define OSH_SIM3_INVERSE    3
#define OSH_SIM3_MAP        4
#define OSH_SIM3_EDGE_ERROR 5
#define OSH_SIM3_OPLUS      6
#define OSH_SIM3_QUAT_TO_R  7
#define OSH_SIM3_R_TO_QUAT  8
#define OSH_SIM3_SOLVE3     9
int osh_host_sim3_apply(int32_t op, int32_t n, const double* a, const double* b, const double* c, const uint8_t* flag, double* out);

/* csrc/pgo4_se3.h (the 4-DoF pose graph's algebra) compiled for the host, applied to n items.  A vertex state is 34 doubles
 * (DR, Rwb, twb, Rcw, tcw row-major, then its), its constants 21 (Rwb0, Rcb, tcb), an edge's measurement 12 (dR, dt).
 *   EXP         a[3] (x y z)                               -> out[9]   ExpSO3
 *   LOG         a[9]                                       -> out[3]   LogSO3
 *   NORMALIZE   a[9]                                       -> out[9]   NormalizeRotation
 *   UPDATE      a = state[34], b = const[21], c = u[4]     -> out[34]  VertexPose4DoF::oplusImpl
 *   EDGE_ERROR  a = meas[12], b = state_i, c = state_j      -> out[6]   Edge4DoF::computeError
 * Returns 0, or -1 for an unknown op or a missing array. */
#define OSH_PGO4_EXP        0
#define OSH_PGO4_LOG        1
#define OSH_PGO4_NORMALIZE  2
#define OSH_PGO4_UPDATE     3
#define OSH_PGO4_EDGE_ERROR 4
int osh_host_pgo4_apply(int32_t op, int32_t n, const double* a, const double* b, const double* c, double* out);
/* out[0] = sizeof(osh_pgo4_problem), out[1] = sizeof(osh_pgo4_result) as the C compiler lays them out */
void osh_host_pgo4_sizes(int64_t* out);

/* ---- Optimizer::OptimizeSim3 (csrc/host/OptimizerSim3.cc) on two stand-in keyframes (csrc/hosttest/sim3opt.cc) ---- */
typedef struct osh_host_sim3_kf {
  float pose[7];                  /* Tcw: qx qy qz qw tx ty tz, returned as is by GetPose()                     */
  float cam[8];                   /* mpCamera->mvParameters: fx fy cx cy, then k1..k4 for a KannalaBrandt8       */
  int32_t kb8;                    /* 1: mpCamera is a KannalaBrandt8, 0: a Pinhole                              */
  int32_t n_keys;
  const float* keys_un;           /* [n_keys*2] mvKeysUn                                                        */
  const int32_t* octave;          /* [n_keys] their octaves                                                     */
  int32_t n_levels;
  const float* inv_level_sigma2;  /* [n_levels] mvInvLevelSigma2                                                */
} osh_host_sim3_kf;

typedef struct osh_host_sim3_input {
  osh_host_sim3_kf kf1, kf2;
  int32_t n_points;
  const float* mp_pos;            /* [n_points*3] world positions                                               */
  const uint8_t* mp_bad;          /* [n_points] isBad()                                                         */
  const int32_t* mp_index2;       /* [n_points] the point's keypoint in pKF2 (GetIndexInKeyFrame), -1: none     */
  const int32_t* mp_track_level;  /* [n_points] mnTrackScaleLevel                                               */
  const int32_t* kf1_mp;          /* [kf1.n_keys] map point of pKF1's slot (GetMapPointMatches), -1: NULL       */
  int32_t n_matches;
  const int32_t* matches1;        /* [n_matches] vpMatches1, -1: NULL                                           */
  double S12[8];                  /* g2oS12 passed in                                                           */
  float th2;
  int32_t fix_scale, all_points;  /* bFixScale, bAllPoints                                                      */
} osh_host_sim3_input;

/* The pair walk alone (PackOptimizeSim3, no device): fills *out, pointing its arrays at the caller's (max_pairs entries each:
 * index, X1c / X2c [3], obs1 / obs2 [2], info1 / info2), and returns the number of pairs; -1 when there are more than max_pairs
 * or a camera is refused. */
struct osh_sim3_problem;
int osh_host_pack_sim3(const osh_host_sim3_input* in, int32_t max_pairs, struct osh_sim3_problem* out, int32_t* index, double* X1c,
                       double* X2c, double* obs1, double* obs2, double* info1, double* info2);
/* Optimizer::OptimizeSim3 itself: returns its value; nulled[n_matches] = 1 where it cleared vpMatches1[i]; S12[8] holds g2oS12 after
 * the call (in->S12 when untouched); hessian[49] is mAcumHessian, read before and written after the call (row-major). */
int osh_host_optimize_sim3(const osh_host_sim3_input* in, uint8_t* nulled, double* S12, double* hessian);

/* ---- Frame::ComputeStereoMatches (src/Frame.cc:816-986; csrc/host/Frame.cc, csrc/hosttest/stereo.cc) ---- */
/* A rectified stereo frame as flat arrays.  The pyramid levels of a side lie one after another in *_pixels, each contiguous
 * (rows[l] * cols[l] bytes, row-major). */
typedef struct osh_host_stereo_input {
  int32_t n_left, n_right;
  const float* left_xy; const int32_t* left_octave; const uint8_t* left_desc;      /* [n_left*2], [n_left], [n_left*32]    */
  const float* right_xy; const int32_t* right_octave; const uint8_t* right_desc;   /* [n_right*2], [n_right], [n_right*32] */
  int32_t n_levels;
  const float* scale_factors; const float* inv_scale_factors;                      /* [n_levels] each                      */
  const int32_t* left_rows; const int32_t* left_cols; const int32_t* right_rows; const int32_t* right_cols;   /* [n_levels] */
  const uint8_t* left_pixels; const uint8_t* right_pixels;
  float bf, b;
} osh_host_stereo_input;
/* The pack alone (PackStereoMatches of csrc/host/host_pack.h, no device) on a stand-in Frame whose pyramid levels are views into
 * images with `border` pixels around them (row stride cols + 2 * border), then read back the way a consumer of osh_stereo_frame
 * reads it: sizes = n_left, n_right, n_levels; scales[2*l] = scale, [2*l+1] = inverse scale; level_shape[(side*n_levels + l)*3] =
 * rows, cols, stride; *_pixels = the levels gathered row by row through data + r * stride.  Every output may be NULL. */
int osh_host_pack_stereo(const osh_host_stereo_input* in, int32_t border, int32_t sizes[3], float* left_xy, int32_t* left_octave,
                         uint8_t* left_desc, float* right_xy, int32_t* right_octave, uint8_t* right_desc, float* scales,
                         int64_t* level_shape, uint8_t* left_pixels, uint8_t* right_pixels, float bf_b[2]);
/* Frame::ComputeStereoMatches itself on such a Frame: u_right = mvuRight, depth = mvDepth ([n_left] each). */
int osh_host_compute_stereo_matches(const osh_host_stereo_input* in, int32_t border, float* u_right, float* depth);
/* A plain single-thread C++ restatement of src/Frame.cc:816-986 with the outputs of osh_stereo_result (all but u_right / depth may be
 * NULL); flags[i] bit 0: the disparity <= 0 branch (0.01) was taken, bit 1: the smallest SAD occurs at more than one increment;
 * undefined[4] counts the inputs on which the reference's behaviour is undefined (defined skips here): row-table entries outside the
 * image, left keypoints whose row is outside, patches that leave their image, 1 if no keypoint was accepted; *ms = its wall time. */
int osh_host_stereo_restatement(const osh_host_stereo_input* in, float* u_right, float* depth, int32_t* best_right, int32_t* hamming,
                                int32_t* sad, int32_t* best_inc, uint8_t* stage, uint8_t* flags, int32_t undefined[4], double* ms);

/* ---- Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1131-1171; csrc/host/Frame.cc, csrc/hosttest/stereo.cc) ---- */
/* A frame of a KannalaBrandt8 rig as flat arrays (the fields of osh_fisheye_stereo_frame). */
typedef struct osh_host_fisheye_input {
  int32_t n_left, n_right, mono_left, mono_right;
  const float* left_xy; const int32_t* left_octave; const uint8_t* left_desc;      /* [n_left*2], [n_left], [n_left*32]    */
  const float* right_xy; const int32_t* right_octave; const uint8_t* right_desc;   /* [n_right*2], [n_right], [n_right*32] */
  int32_t n_levels;
  const float* level_sigma2;                                                       /* [n_levels] mvLevelSigma2             */
  float cam1[8], cam2[8], precision1, precision2, Rlr[9], tlr[3];
} osh_host_fisheye_input;
/* Frame::ComputeStereoFishEyeMatches itself on a stand-in Frame made of it (mpCamera / mpCamera2 = KannalaBrandt8 with the given
 * precision, mRlr / mtlr as given; camera2_pinhole != 0: mpCamera2 is a Pinhole instead, which the body refuses with a message).
 * Outputs (each may be NULL): mvLeftToRightMatch, mvRightToLeftMatch, mvDepth, mvStereo3Dpoints [n_left*3], mvuRight. */
int osh_host_compute_fisheye_stereo_matches(const osh_host_fisheye_input* in, int32_t camera2_pinhole, int32_t* left_to_right,
                                            int32_t* right_to_left, float* depth, float* p3d, float* u_right);
/* csrc/kb8_triangulate.h (the device's KannalaBrandt8::TriangulateMatches) compiled for the host, arguments as osh_kb8_triangulate
 * without a context; no output may be NULL. */
struct osh_kb8_rig;
int osh_host_kb8_triangulate_cpu(int32_t n, const struct osh_kb8_rig* rig, const float* xy1, const float* xy2, const float* sigma1,
                                 const float* sigma2, float* ret, float* p3d, float* cos_parallax);

/* ---- LocalMapping::CreateNewMapPoints (include/LocalMapping.h, csrc/host/LocalMapping.cc, csrc/hosttest/newpoints.cc) ---- */
struct osh_newpoint_segment;
struct osh_newpoint_result;
/* csrc/newpoint_triangulate.h (the statements k_newpoint_triangulate runs per match) compiled for the host, on one thread: arguments
 * as osh_orb_triangulate_new_points without a context and without its validation (the segments must be valid).  *ms (may be NULL) =
 * wall time of the loop over the matches.  -1: bad arguments. */
int osh_host_newpoint_triangulate_cpu(int32_t n_segments, const struct osh_newpoint_segment* segments,
                                      const struct osh_newpoint_result* results, double* ms);

/* A keyframe of the stand-in class from flat arrays.  n_left < 0: mvKeysUn = mvKeys = the n keypoints; else a rig keyframe, the
 * first n_left keypoints in mvKeys, the rest in mvKeysRight.  Feature i holds a map point at mp_pos[i] already when has_mp[i].
 * mFeatVec as CSR (node ids ascending).  The level tables are scale_factor^level and its square by repeated float multiplication. */
typedef struct osh_host_newpoint_kf {
  int32_t n, n_left;
  const float* xy;            /* [n*2]  */
  const int32_t* octave;      /* [n]    */
  const uint8_t* desc;        /* [n*32] */
  const float* u_right;       /* [n] mvuRight */
  const float* depth;         /* [n] mvDepth  */
  const uint8_t* has_mp;      /* [n]    */
  const float* mp_pos;        /* [n*3]  */
  int32_t n_nodes;
  const int32_t* node_id;     /* [n_nodes]   */
  const int32_t* node_off;    /* [n_nodes+1] */
  const int32_t* node_feat;
  float pose_qt[7];           /* Tcw: qx qy qz qw tx ty tz */
  float trl_qt[7];            /* mTrl (rig only)           */
  int32_t camera_kb8;         /* mpCamera: 0 Pinhole, 1 KannalaBrandt8 */
  float camera[8];
  int32_t has_camera2;        /* mpCamera2: a KannalaBrandt8 */
  float camera2[8];
  float mbf, mb;
  int32_t n_levels;
  float scale_factor;
  int32_t prev;               /* mPrevKF as an index into the scene's keyframes, -1: none */
} osh_host_newpoint_kf;
typedef struct osh_host_newpoint_scene {
  int32_t n_kf;
  const osh_host_newpoint_kf* kf;      /* kf[0] is mpCurrentKeyFrame */
  int32_t n_neighbours;
  const int32_t* neighbours;           /* its covisibles, best first, as indices into kf */
  int32_t monocular, inertial, far_points;
  float th_far_points;
  int32_t recently_lost;               /* mpTracker->mState == Tracking::RECENTLY_LOST */
  int32_t inertial_ba2;                /* Map::GetIniertialBA2()                        */
  int32_t new_keyframe_waiting;        /* CheckNewKeyFrames() returns true              */
} osh_host_newpoint_scene;
/* LocalMapping::CreateNewMapPoints on the scene.  Returns the number of map points created (in mlpRecentAddedMapPoints order) and,
 * for the first `capacity` of them: the neighbour (index into kf), idx1, idx2, the position [3], nObs, and flags: bit 0 / 1 the
 * slot idx1 of the current keyframe / idx2 of the neighbour holds the point, bit 2 / 3 its observation of the current keyframe /
 * the neighbour names idx1 / idx2 (in the right-camera slot of the tuple for a right keypoint of a rig), bit 4
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth ran once each, bit 5 the map lists it, bit 6 its reference keyframe is the
 * current one.  poses (may be NULL) [n_kf*48]: Rcw tcw Rwc Ow of the left and of the right pose of every keyframe as the pack hands
 * them to the device (the right one only for a rig).  -1: bad arguments. */
int osh_host_create_new_map_points(const osh_host_newpoint_scene* scene, int32_t capacity, int32_t* neighbour, int32_t* idx1, int32_t* idx2,
                                   float* x3d, int32_t* n_obs, int32_t* flags, float* poses);

/* ---- TwoViewReconstruction (include/TwoViewReconstruction.h, csrc/host/TwoViewReconstruction.cc, csrc/hosttest/two_view.cc) ---- */
struct osh_two_view_problem;
struct osh_two_view_result;
/* csrc/two_view.h (the statements of two_view_device.hip) compiled for the host, on one thread: arguments as
 * osh_orb_two_view_reconstruct without a context, without its validation (the problems must be valid) and without its limits.
 * *ms (may be NULL) = wall time of the call.  -1: bad arguments. */
int osh_host_two_view_cpu(int32_t n_problems, const struct osh_two_view_problem* problems, const struct osh_two_view_result* results,
                          double* ms);
/* Normalize (src/TwoViewReconstruction.cc:737-784) of csrc/two_view.h over the n keypoints xy [n*2]: pn [n*2], T [9] row-major. */
int osh_host_two_view_normalize(int32_t n, const float* xy, float* pn, float* T);
/* The decision of ReconstructF (branch 0, n_good / parallax [4]) or ReconstructH (branch 1, [8]) on N inliers: returns the
 * OSH_TWOVIEW_* status, *winner = the hypothesis it reports (-1: none).  -1: bad arguments. */
int osh_host_two_view_decide(int32_t branch, int32_t n_inliers, const int32_t* n_good, const float* parallax, int32_t* winner);
/* The motion hypotheses of ReconstructH (branch 1, model = H21 [9]: :582-690) or of ReconstructF / DecomposeE (branch 0, model = F21:
 * :484-493,903-927) for K [9]: R [8*9], t [8*3].  Returns their number: 8, 4, or 0 when ReconstructH's 1.00001 test refuses.  -1: bad
 * arguments. */
int osh_host_two_view_motion(int32_t branch, const float* model, const float* K, float* R, float* t);
/* camera 0: TwoViewReconstruction(K = params[9], sigma, iterations).Reconstruct; 1: Pinhole(params[4]).ReconstructWithTwoViews;
 * 2: KannalaBrandt8(params[8]).ReconstructWithTwoViews (both with the class defaults sigma 1, 200 iterations; pass iterations = 200).
 * xy1 [n1*2], xy2 [n2*2], matches12 [n1] (-1: unmatched).  vP3D and vbTriangulated go in with *n_p3d / *n_triangulated entries
 * (p3d [max(*n_p3d, n1)*3] holds the incoming points) and come back with the sizes Reconstruct left and their first n1 entries.
 * T21 [12]; sets [iterations*8] = mvSets; info [3] = status, 1 if the device answered, mvSets.size().  Returns 1 / 0 as
 * Reconstruct, -1: bad arguments. */
int osh_host_two_view_reconstruct(int32_t camera, const float* params, float sigma, int32_t iterations, int32_t n1, const float* xy1,
                                  int32_t n2, const float* xy2, const int32_t* matches12, float* T21, float* p3d, int32_t* n_p3d,
                                  uint8_t* triangulated, int32_t* n_triangulated, int32_t* sets, int32_t* info);

/* ---- MLPnP, the PnP RANSAC of relocalisation (csrc/mlpnp.h, csrc/hosttest/mlpnp.cc) ---- */
struct osh_mlpnp_problem;
struct osh_mlpnp_result;
/* csrc/mlpnp.h (the statements of mlpnp_device.hip) compiled for the host, on one thread: arguments as osh_orb_mlpnp_solve without a
 * context, without its validation (the problems must be valid) and without its limits.  *ms (may be NULL) = wall time of the call.
 * -1: bad arguments. */
int osh_host_mlpnp_cpu(int32_t n_problems, const struct osh_mlpnp_problem* problems, const struct osh_mlpnp_result* results, double* ms);
/* CheckInliers of csrc/mlpnp.h: arguments as osh_orb_mlpnp_check_inliers without a context. */
int osh_host_mlpnp_check_inliers(const struct osh_mlpnp_problem* problem, int32_t n_poses, const double* poses, int32_t* count, uint32_t* mask);
/* The stages of computePose, one by one.  nullspace: N [3*2] row-major for the bearing vector f [3].  rank: the rank of the symmetric
 * S [9] as the planarity test counts it.  null_vector: the null vector h [cols] of the symmetric M [cols*cols], cols 9 or 12.
 * compute_pose: computePose over n >= 6 correspondences (bearing, p3d [n*3]): pose [12], info [3] (may be NULL) = planar,
 * Gauss-Newton updates applied, how it ended (0: its bound, 1: the break on dx, 2: the stop on J dx).  gauss_newton: mlpnp_gn from
 * x [6] (omega, t; updated in place) with at most max_iterations rounds: info [2] = updates applied, how it ended.  -1: bad arguments. */
int osh_host_mlpnp_nullspace(const double* f, double* N);
int osh_host_mlpnp_rank(const double* S);
int osh_host_mlpnp_null_vector(const double* M, int32_t cols, double* h);
int osh_host_mlpnp_compute_pose(int32_t n, const double* bearing, const double* p3d, double* pose, int32_t* info);
int osh_host_mlpnp_gauss_newton(int32_t n, const double* bearing, const double* p3d, double* x, int32_t max_iterations, int32_t* info);
/* SetRansacParameters (src/MLPnPsolver.cpp:225-260) of csrc/mlpnp.h for n correspondences: out [2] = mRansacMinInliers, mRansacMaxIts. */
int osh_host_mlpnp_ransac_parameters(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set, float epsilon,
                                     int32_t* out);
/* The record scan and the decision of csrc/mlpnp.h from per-iteration counts and per-record refined counts (record_count
 * [n_iterations], read for the records that occur): record [n_iterations] gets the record iterations; out [7] = first_hit,
 * hit_record, hit_count, best_iteration, best_count, best_refine_ok, n_records.  -1: bad arguments. */
int osh_host_mlpnp_replay(int32_t n_iterations, const int32_t* count, int32_t min_inliers, int32_t best_inliers_in, int32_t best_refine_ok_in,
                          const int32_t* record_count, int32_t* record, int32_t* out);

/* An MLPnPsolver (include/MLPnPsolver.h, csrc/host/MLPnPsolver.cc) of the stand-in classes: camera_type 0 Pinhole(params[4]), 1
 * KannalaBrandt8(params[8]); a Frame with n_keys undistorted keypoints (xy [n_keys*2], octave [n_keys]) and level_sigma2 [n_levels];
 * vpMapPointMatches of n_matches entries, state [n_matches] 0 none, 1 a map point at world [i*3], 2 a bad one.  NULL: bad arguments. */
void* osh_host_mlpnp_solver_create(int32_t camera_type, const float* params, int32_t n_keys, const float* xy, const int32_t* octave,
                                   int32_t n_levels, const float* level_sigma2, int32_t n_matches, const float* world, const uint8_t* state);
void osh_host_mlpnp_solver_destroy(void* solver);
int osh_host_mlpnp_solver_set_ransac(void* solver, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set,
                                     float epsilon, float th2);
/* out [7] = N, mRansacMinInliers, mRansacMaxIts, mnIterations, mnBestInliers, queued sets, 1 if the device answered the last iterate */
int osh_host_mlpnp_solver_state(void* solver, int32_t* out);
/* iterate(n_iterations, ..) of every solver, one by one (batch 0) or through MLPnPsolver::IterateBatch (batch 1).  Per solver:
 * found, no_more, n_inliers, inliers [n_matches + 1] (vbInliers cut to n_matches; the last byte: 1 if vbInliers is not empty),
 * Tout [16] row-major.  -1: bad arguments. */
int osh_host_mlpnp_solver_iterate(int32_t n_solvers, void* const* solvers, int32_t n_iterations, int32_t batch, int32_t n_matches,
                                  uint8_t* found, uint8_t* no_more, int32_t* n_inliers, uint8_t* inliers, float* Tout);
/* The two halves of iterate around the device call.  prepare: draws (or takes from the queue) the sets of one iterate(n_iterations):
 * returns their number and the first `capacity` of them in sets [capacity*6]; -2 when N < mRansacMinInliers.  replay: walks a given
 * answer for the prepared round: head [6] = first_hit, hit_record, hit_count, best_iteration, best_count, best_refine_ok; poses
 * [12], masks [OSH_MLPNP_MASK_WORDS(N)]; outputs as iterate's.  Returns iterate's return value; -1: bad arguments. */
int osh_host_mlpnp_solver_prepare(void* solver, int32_t n_iterations, int32_t capacity, int32_t* sets);
int osh_host_mlpnp_solver_replay(void* solver, const int32_t* head, const double* hit_pose, const uint32_t* hit_mask, const double* best_pose,
                                 const uint32_t* best_mask, int32_t n_matches, uint8_t* no_more, int32_t* n_inliers, uint8_t* inliers,
                                 float* Tout);

/* ---- Sim3Solver, the Sim3 RANSAC of loop closing (csrc/sim3_ransac.h, csrc/hosttest/sim3solver.cc) ---- */
struct osh_sim3r_problem;
struct osh_sim3r_result;
/* csrc/sim3_ransac.h (the statements of sim3_ransac_device.hip) compiled for the host, on one thread: arguments as
 * osh_orb_sim3_ransac without a context, without its validation (the problems must be valid) and without its limits.  *ms (may be
 * NULL) = wall time of the call.  -1: bad arguments. */
int osh_host_sim3r_cpu(int32_t n_problems, const struct osh_sim3r_problem* problems, const struct osh_sim3r_result* results, double* ms);
/* CheckInliers of csrc/sim3_ransac.h: arguments as osh_orb_sim3_ransac_check_inliers without a context. */
int osh_host_sim3r_check_inliers(const struct osh_sim3r_problem* problem, int32_t n_T, const float* T12s, int32_t* count, uint32_t* mask);
/* ComputeSim3 of one minimal set: P1, P2 [9] = the three members in camera 1 and camera 2 (point after point), T13 [13] = R, t, s. */
int osh_host_sim3r_compute_sim3(const float* P1, const float* P2, int32_t fix_scale, float* T13);
/* The record scan from per-iteration counts: record [n_iterations] gets the record iterations; out [4] = first_hit, n_records,
 * best_iteration, best_count.  -1: bad arguments. */
int osh_host_sim3r_scan(int32_t n_iterations, const int32_t* count, int32_t min_inliers, int32_t best_inliers_in, int32_t* record, int32_t* out);
/* mRansacMaxIts of SetRansacParameters (src/Sim3Solver.cc:123-147) for n correspondences. */
int osh_host_sim3r_max_iterations(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations);
/* A Sim3Solver (include/Sim3Solver.h, csrc/host/Sim3Solver.cc) of the stand-in classes.  Keyframe 0 is pKF1, 1 is pKF2, 2 (n_kf = 3)
 * one more keyframe a point may be matched in.  Map points by world position, isBad() and their keypoint index in each keyframe
 * (GetIndexInKeyFrame, -1: not observed).  pKF1's GetMapPointMatches() has n1 slots (kf1_mp: a point or -1); vpMatched12 has n1
 * entries (matched12: a point or -1); matched_kf [n1]: vpKeyFrameMatchedMP as keyframe indices, or NULL: passed empty. */
typedef struct osh_host_sim3_scene {
  int32_t n_kf;
  int32_t camera_type[3];         /* 0 Pinhole (4 parameters), 1 KannalaBrandt8 (8)                                  */
  float camera[3][8];
  float Rcw[3][9], tcw[3][3];     /* GetRotation() (row-major, the entries as given), GetTranslation()                */
  int32_t n_keys[3];
  const float* xy[3];             /* [n_keys*2] mvKeysUn                                                             */
  const int32_t* octave[3];       /* [n_keys]                                                                        */
  int32_t n_levels;
  const float* level_sigma2;      /* [n_levels] mvLevelSigma2 of every keyframe                                      */
  int32_t n_points;
  const float* world;             /* [n_points*3]                                                                    */
  const uint8_t* bad;             /* [n_points]                                                                      */
  const int32_t* index_in_kf;     /* [n_points*3]                                                                    */
  int32_t n1;
  const int32_t* kf1_mp;          /* [n1]                                                                            */
  const int32_t* matched12;       /* [n1]                                                                            */
  const int32_t* matched_kf;      /* [n1] or NULL                                                                    */
  int32_t fix_scale;
} osh_host_sim3_scene;
void* osh_host_sim3_solver_create(const osh_host_sim3_scene* scene);
void osh_host_sim3_solver_destroy(void* solver);
int osh_host_sim3_solver_set_ransac(void* solver, double probability, int32_t min_inliers, int32_t max_iterations);
/* out [8] = N, mN1, mRansacMinInliers, mRansacMaxIts, mnIterations, mnBestInliers, 1 if an answer is kept, 1 if the device gave it */
int osh_host_sim3_solver_state(void* solver, int32_t* out);
/* The constructor's pack, N entries each: mvX3Dc1/2 [N*3], mvP1im1 / mvP2im2 [N*2], (float)mvnMaxError1/2 [N], mvnIndices1 [N]. */
int osh_host_sim3_solver_pack(void* solver, float* x3dc1, float* x3dc2, float* p1im1, float* p2im2, float* max_error1, float* max_error2,
                              int32_t* indices1);
/* GetEstimatedTransformation [16], Rotation [9], Translation [3], Scale, mvbBestInliers [N]. */
int osh_host_sim3_solver_best(void* solver, float* T12, float* R, float* t, float* scale, uint8_t* flags);
/* Every solver once.  mode 0: iterate(n_iterations, bNoMore, vbInliers, nInliers); 1: the overload with bConverge; 2: all through
 * Sim3Solver::IterateBatch; 3: find.  Per solver: no_more, n_inliers, converged, inliers [n1] (vbInliers cut to n1), Tout [16]
 * row-major.  -1: bad arguments. */
int osh_host_sim3_solver_iterate(int32_t n_solvers, void* const* solvers, int32_t n_iterations, int32_t mode, int32_t n1, uint8_t* no_more,
                                 int32_t* n_inliers, uint8_t* converged, uint8_t* inliers, float* Tout);
/* The two halves of iterate around the device call.  prepare: the sets the call would run, their number returned (0: no call is
 * due) and the first `capacity` of them in sets [capacity*3].  keep: a given answer for the prepared round (the records only).
 * replay: nIterations iterations from the kept answer, outputs as iterate's for one solver. */
int osh_host_sim3_solver_prepare(void* solver, int32_t capacity, int32_t* sets);
int osh_host_sim3_solver_keep(void* solver, int32_t n_records, const int32_t* record, const int32_t* record_count, const float* record_T,
                              const uint32_t* record_mask);
int osh_host_sim3_solver_replay(void* solver, int32_t n_iterations, int32_t five, int32_t n1, uint8_t* no_more, int32_t* n_inliers,
                                uint8_t* converged, uint8_t* inliers, float* Tout);

/* ---- ORBextractor::ComputeKeyPointsOctTree (include/ORBextractor.h, csrc/host/ORBextractor.cc, csrc/hosttest/orbextractor.cc) ---- */
struct osh_fast_frame;
struct osh_fast_result;
struct osh_ic_angle_frame;
struct osh_ic_angle_result;
/* csrc/orb_fast.h (the statements k_fast_cells, k_fast_emit and k_ic_angle run) compiled for the host, on one thread: arguments as
 * osh_orb_fast_detect / osh_orb_ic_angle without a context and without their validation (the frames must be valid and bring their
 * pyramid; pyramid_token comes back 0).  *ms (may be NULL) = wall time of the loops.  -1: bad arguments. */
int osh_host_orb_fast_cpu(int32_t n_frames, const struct osh_fast_frame* frames, struct osh_fast_result* results, double* ms);
int osh_host_orb_ic_angle_cpu(int32_t n_frames, const struct osh_ic_angle_frame* frames, const struct osh_ic_angle_result* results, double* ms);
/* The cell geometry of csrc/orb_fast.h for a level of rows x cols pixels: geom[0..5] = nCols, nRows, wCell, hCell, maxBorderX,
 * maxBorderY (nCols = nRows = 0: no cells), and the rectangle x0, y0, w, h of each existing cell in (i, j) order in rects (may be
 * NULL, else room for nCols * nRows * 4).  Returns the number of existing cells.  -1: bad arguments. */
int osh_host_orb_fast_level_cells(int32_t rows, int32_t cols, int32_t geom[6], int32_t* rects);

/* An ORBextractor of the stand-in class, ORBextractor(nfeatures, scale_factor, nlevels, ini_th, min_th), with the n_images levels
 * (nlevels of them, or fewer to see the refusal) stored as views into images with `border` pixels around them. */
typedef struct osh_host_orbextractor_input {
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels, ini_th, min_th;
  int32_t n_images;
  const int32_t* rows;        /* [n_images] */
  const int32_t* cols;        /* [n_images] */
  const uint8_t* pixels;      /* the levels one after another, rows packed */
  int32_t border;
} osh_host_orbextractor_input;
typedef struct osh_host_orbextractor_output {
  int32_t capacity, cand_capacity;
  int32_t* level_count;       /* [nlevels] allKeypoints[level].size()                                                 */
  float* xy;                  /* [capacity*2] allKeypoints level after level: pt                                      */
  float* response;            /* [capacity] */
  float* angle;               /* [capacity] */
  float* size;                /* [capacity] */
  int32_t* octave;            /* [capacity] */
  int32_t* cand_level_count;  /* [nlevels] vToDistributeKeys.size() of the level's DistributeOctTree call (0: no call) */
  float* cand_xy;             /* [cand_capacity*2] the vToDistributeKeys of the calls, level after level               */
  float* cand_response;       /* [cand_capacity] */
  int32_t* cand_args;         /* [nlevels*6] minX maxX minY maxY nFeatures level of the level's call; may be NULL      */
  int32_t* features_per_level;/* [nlevels] mnFeaturesPerLevel; may be NULL                                            */
  float* scale_factors;       /* [nlevels] mvScaleFactor; may be NULL                                                 */
} osh_host_orbextractor_output;
/* ORBextractor::ComputeKeyPointsOctTree on that extractor.  Returns the number of keypoints of all levels (the arrays take the
 * first `capacity` keypoints and `cand_capacity` candidates).  -1: bad arguments, -2: the member left something inconsistent. */
int osh_host_orbextractor_compute_keypoints(const osh_host_orbextractor_input* in, const osh_host_orbextractor_output* out);

/* ---- ORBextractor::DistributeOctTree (csrc/orb_octree.h, csrc/host/ORBextractor.cc, csrc/hosttest/octree.cc) ---- */
struct osh_octree_list;
struct osh_octree_result;
/* csrc/orb_octree.h compiled for the host, on one thread (osh::octree_distribute_host): arguments, checks, return codes and the
 * overflow convention of osh_orb_octree_distribute without a context; the limits on n_features, candidates and roots are those of
 * the device call although the host statements have none.  *ms (may be NULL) = wall time of the lists without the checks. */
int osh_host_orb_octree_cpu(int32_t n_lists, const struct osh_octree_list* lists, struct osh_octree_result* results, double* ms);
/* ORBextractor::DistributeOctTreeDevice of a stand-in extractor on the candidates of `list` with minX = minY = 16, maxX = 16 + width,
 * maxY = 16 + height: index [capacity] receives the input index of each kept keypoint in result order (carried through
 * cv::KeyPoint::class_id), xy [capacity*2] and response [capacity] (each may be NULL) the kept keypoints themselves,
 * *distribute_calls the number of DistributeOctTree calls the member made (the test double records them).  Returns the number of kept keypoints.  -1: bad arguments. */
int osh_host_orbextractor_distribute_device(const struct osh_octree_list* list, int32_t capacity, int32_t* index, float* xy, float* response,
                                            int32_t* distribute_calls);

/* ORBextractor::ExtractBatch of n stand-in extractors ORBextractor(nfeatures, scale_factor, nlevels, ini_th, min_th), one per
 * input (an input with rows == 0 is an empty image; `lapping` is its vLappingArea), with bKeepPyramid = keep_pyramid.  Output i
 * (capacity, pixel_capacity, xy, angle, size, response, octave, descriptors, ret, desc_rows, level_rows, level_cols, pyramid and
 * pixels_needed as osh_host_orbextractor_extract fills them, the levels being mvImagePyramid after the call) and tokens[i] =
 * mnPyramidToken.  Returns 0.  -1: bad arguments. */
struct osh_host_extract_input;
struct osh_host_extract_output;
int osh_host_orbextractor_extract_batch(int32_t n, const struct osh_host_extract_input* in, const struct osh_host_extract_output* out,
                                        int32_t keep_pyramid, uint64_t* tokens);

/* ---- ORBextractor::operator() (csrc/orb_brief.h, csrc/host/ORBextractor.cc, csrc/hosttest/orbextractor.cc) ---- */
struct osh_describe_frame;
struct osh_describe_result;
/* csrc/orb_brief.h (the statements k_orb_blur and k_orb_brief run) compiled for the host, on one thread: arguments as
 * osh_orb_describe without a context and without its validation (the frames must be valid and bring their pyramid).  *ms (may be
 * NULL) = wall time of the loops.  -1: bad arguments. */
int osh_host_orb_describe_cpu(int32_t n_frames, const struct osh_describe_frame* frames, const struct osh_describe_result* results, double* ms);
/* brief_gaussian_q8 of csrc/orb_brief.h: the ksize (odd, at most 31) Q8 weights of sigma into out.  -1: bad arguments. */
int osh_host_brief_gaussian_q8(int32_t ksize, double sigma, uint16_t* out);
/* brief_reach of csrc/orb_brief.h for a table of 512 points. */
int osh_host_brief_reach(const int8_t* pattern);
/* The table the stand-in constructor generates (its own: 512 points in [-13, 12]^2 with radius at most 18.38) into pattern[1024]. */
int osh_host_orbextractor_pattern(int8_t* pattern);

/* ORBextractor(nfeatures, scale_factor, nlevels, ini_th, min_th)(image, mask, keypoints, descriptors, lapping_area) of the stand-in
 * class on a rows x cols image (rows == 0: an empty image). */
typedef struct osh_host_extract_input {
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels, ini_th, min_th;
  int32_t rows, cols;
  const uint8_t* pixels;      /* rows packed */
  int32_t lapping[2];         /* vLappingArea */
} osh_host_extract_input;
typedef struct osh_host_extract_output {
  int32_t capacity;           /* keypoints the arrays below can take */
  int32_t pixel_capacity;     /* bytes pyramid can take */
  int32_t* level_rows;        /* [nlevels] the pyramid ComputePyramid built */
  int32_t* level_cols;        /* [nlevels] */
  uint8_t* pyramid;           /* its levels one after another, rows packed */
  int32_t* level_count;       /* [nlevels] allKeypoints[level].size() of ComputeKeyPointsOctTree */
  float* level_xy;            /* [capacity*2] allKeypoints level after level, in the pixels of their level */
  float* level_angle;         /* [capacity] */
  float* xy;                  /* [capacity*2] _keypoints */
  float* angle;               /* [capacity] */
  float* size;                /* [capacity] */
  float* response;            /* [capacity] */
  int32_t* octave;            /* [capacity] */
  uint8_t* descriptors;       /* [capacity*32] _descriptors */
  int32_t* ret;               /* the return value (monoIndex, -1 for an empty image) */
  int32_t* desc_rows;         /* _descriptors.rows after the call (0: released) */
  int32_t* pixels_needed;     /* bytes of the pyramid */
  double* call_ms;            /* wall time of the operator() call alone; may be NULL */
} osh_host_extract_output;
/* Returns _keypoints.size() (the arrays are filled when it and the pyramid fit the capacities).  -1: bad arguments. */
int osh_host_orbextractor_extract(const osh_host_extract_input* in, const osh_host_extract_output* out);

/* ---- ORBextractor::ComputePyramid (csrc/orb_pyramid.h, csrc/host/ORBextractor.cc, csrc/hosttest/orbextractor.cc) ---- */
struct osh_pyramid_frame;
struct osh_pyramid_result;
/* csrc/orb_pyramid.h (the statements k_pyr_level and k_pyr_border run) compiled for the host, on one thread: arguments as
 * osh_orb_pyramid_build without a context; pyramid_token comes back 0.  What that call refuses is refused here with the same code
 * (OSH_ERR_INVALID / OSH_ERR_UNSUPPORTED) and no message.  *ms (may be NULL) = wall time of the loops.  -1: bad arguments. */
int osh_host_orb_pyramid_cpu(int32_t n_frames, const struct osh_pyramid_frame* frames, struct osh_pyramid_result* results, double* ms);
/* ORBextractor::ComputePyramid of the stand-in class on the image of `in` (lapping is not read), then ComputeKeyPointsOctTree right
 * after it (which consumes mnBuiltPyramidToken) and once more after mvImagePyramid has been replaced by a hand-set copy of itself. */
typedef struct osh_host_pyramid_output {
  int32_t capacity;           /* keypoints each of the two sets of arrays can take */
  int32_t pixel_capacity;     /* bytes `bordered` can take */
  int32_t* level_rows;        /* [nlevels] mvImagePyramid[l].rows */
  int32_t* level_cols;        /* [nlevels] */
  uint8_t* bordered;          /* the whole bordered images, (rows + 38) x (cols + 38) each, one after another; may be NULL */
  int32_t* pixels_needed;     /* [1] bytes of all bordered images */
  uint64_t* built_token;      /* [2] mnBuiltPyramidToken after ComputePyramid, and after the first ComputeKeyPointsOctTree */
  int32_t* level_count;       /* [nlevels] allKeypoints[level].size() right after ComputePyramid */
  float* xy;                  /* [capacity*2] in the pixels of their level; may be NULL */
  float* angle;               /* [capacity] may be NULL */
  float* response;            /* [capacity] may be NULL */
  int32_t* hand_level_count;  /* the same from the hand-set copy */
  float* hand_xy;
  float* hand_angle;
  float* hand_response;
} osh_host_pyramid_output;
/* Returns the larger of the two keypoint counts.  -1: bad arguments, -2: the member left something inconsistent. */
int osh_host_orbextractor_compute_pyramid(const osh_host_extract_input* in, const osh_host_pyramid_output* out);

/* ---- the image front end (csrc/orb_prepare.h, csrc/hosttest/prepare.cc) ---- */
struct osh_prepare_frame;
struct osh_prepare_result;
struct osh_rectify_map_desc;
/* csrc/orb_prepare.h (the statements k_prepare runs) compiled for the host, on one thread: frames and results as osh_orb_prepare
 * without a context, except that a frame's rectify map is the host descriptor maps[k] (NULL: no map; `maps` itself may be NULL) and
 * frames[k].map must be NULL: a resident map needs a device.  What osh_orb_prepare and osh_rectify_map_create refuse is refused
 * here with the same code (OSH_ERR_INVALID / OSH_ERR_UNSUPPORTED) and no message; every result must name a gray image.  *ms (may be
 * NULL) = wall time of the loops.  -1: bad arguments. */
int osh_host_orb_prepare_cpu(int32_t n_frames, const struct osh_prepare_frame* frames, const struct osh_rectify_map_desc* const* maps,
                             struct osh_prepare_result* results, double* ms);

/* ORBextractor::ExtractBatchRaw of n stand-in extractors (made from in[i] as osh_host_orbextractor_extract_batch makes them; the
 * rows, cols and pixels of in[i] are not read) on the raw images raw[i], each with an ImagePrep of its own and, when it names maps,
 * a RectifyMap of its own made for the image's size.  Outputs and tokens as osh_host_orbextractor_extract_batch.  gray (may be
 * NULL): the call passes pvGray, and image i of it is written to gray[i] (rows packed, when gray[i] is not NULL and its
 * gray_capacity[i] bytes suffice) with its size in gray_rows[i] / gray_cols[i] (0, 0: pvGray[i] came back empty).  Returns 0.
 * -1: bad arguments. */
typedef struct osh_host_raw_image {
  int32_t rows, cols, channels;   /* rows == 0: an empty image */
  const uint8_t* pixels;          /* rows packed, channels interleaved */
  int32_t rgb;                    /* ImagePrep::bRGB */
  int32_t map_rows, map_cols;     /* of map_x / map_y */
  const float* map_x;             /* rows packed; NULL: ImagePrep::pMap is null */
  const float* map_y;
  int32_t new_rows, new_cols;     /* ImagePrep::newRows, newCols */
} osh_host_raw_image;
int osh_host_orbextractor_extract_batch_raw(int32_t n, const struct osh_host_extract_input* in, const osh_host_raw_image* raw,
                                            const struct osh_host_extract_output* out, int32_t keep_pyramid, uint64_t* tokens,
                                            uint8_t* const* gray, const int32_t* gray_capacity, int32_t* gray_rows, int32_t* gray_cols);

/* Frame::ExtractAndMatchStereo of a stand-in Frame (mbf = bf, mb = b, the scale factors of the left extractor) whose left and right
 * extractors are made from in[0] and in[1] as osh_host_orbextractor_extract_batch makes them.  raw NULL: the grey form on the images
 * of in[0] / in[1]; else the raw form on raw[0] / raw[1], each with an ImagePrep (and RectifyMap) of its own as
 * osh_host_orbextractor_extract_batch_raw makes them.  chain != 0: the same frame through the two calls the member replaces,
 * ExtractBatch or ExtractBatchRaw with bKeepPyramid = true and the lapping areas {0, 0}, then ComputeStereoMatches.  out[0] / out[1]
 * receive mvKeys / mDescriptors and mvKeysRight / mDescriptorsRight with the extractors' pyramids (ret = 0), tokens[0..1] the
 * extractors' mnPyramidToken, n[0..3] = N, mvuRight.size(), mvDepth.size(), mvKeysRight.size(), u_right / depth [u_capacity]
 * mvuRight / mvDepth when they fit, gray .. gray_cols (may be NULL; raw form only) the images of pvGray as
 * osh_host_orbextractor_extract_batch_raw returns them, *call_ms (may be NULL) the wall time of the member calls alone.  Before the
 * call the frame holds three keypoints, mvuRight and mvDepth of three sevens: what the member must replace.  Returns 0.
 * -1: bad arguments or descriptors that do not fit the keypoints. */
int osh_host_frame_extract_and_match_stereo(const struct osh_host_extract_input* in, const osh_host_raw_image* raw, float bf, float b, int32_t chain,
                                            const struct osh_host_extract_output* out, uint64_t* tokens, int32_t u_capacity, float* u_right, float* depth,
                                            int32_t* n, uint8_t* const* gray, const int32_t* gray_capacity, int32_t* gray_rows, int32_t* gray_cols,
                                            double* call_ms);

/* ---- ORBVocabulary / ComputeBoW (include/ORBVocabulary.h, csrc/host/ORBVocabulary.cc, csrc/hosttest/bow.cc) ---- */
struct osh_bow_tree;
struct osh_bow_result;
/* TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259) restated in one thread with std::map
 * vectors, on n descriptors; every output of osh_bow_result, stage outputs included.  -1: bad arguments or a tree
 * osh_bow_tree_check refuses, -2: L2_NORM scoring.  *ms = wall time of the transform without the construction of the nodes. */
int osh_host_bow_restatement(const struct osh_bow_tree* tree, int32_t levelsup, int32_t n, const uint8_t* desc,
                             const struct osh_bow_result* out, double* ms);
/* An ORB_SLAM3::ORBVocabulary behind a handle; NULL when loadFromTextFile returns false. */
typedef struct osh_host_bow_vocab osh_host_bow_vocab;
osh_host_bow_vocab* osh_host_bow_vocab_load(const char* path);
void osh_host_bow_vocab_free(osh_host_bow_vocab* h);
/* Its getters and tree: info = getBranchingFactor, getDepthLevels, getWeightingType, getScoringType, nodes besides the root, size,
 * empty; the four arrays of osh_bow_tree (each may be NULL; call once with NULLs for the sizes) and getParentNode(w, levelsup) of
 * every word w. */
int osh_host_bow_vocab_tree(const osh_host_bow_vocab* h, int32_t info[7], int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight,
                            int32_t levelsup, int32_t* word_parent);
/* Frame::ComputeBoW (keyframe == 0) or KeyFrame::ComputeBoW on a stand-in whose mDescriptors are the n descriptors; mBowVec and
 * mFeatVec come back as the first seven arrays of osh_bow_result.  second_desc != NULL: mDescriptors are then replaced by it and
 * ComputeBoW runs once more (its guard has to keep the vectors).  n_threads > 1: that many threads do the same at once, each on a
 * stand-in of its own; -3 if their results differ. */
int osh_host_bow_compute(osh_host_bow_vocab* h, int32_t keyframe, int32_t n, const uint8_t* desc, const uint8_t* second_desc, int32_t n_threads,
                         const struct osh_bow_result* out);
/* ORBVocabulary::score of two BowVectors given as (word id, value) lists. */
double osh_host_bow_score(int32_t n1, const int32_t* id1, const double* value1, int32_t n2, const int32_t* id2, const double* value2);

/* ---- KeyFrameDatabase (include/KeyFrameDatabase.h, csrc/host/KeyFrameDatabase.cc, csrc/hosttest/kfdb.cc) ---- */
/* A stand-in graph from flat arrays: keyframes with their BowVector, map, bad flag, weight-ordered covisibles
 * (GetBestCovisibilityKeyFrames reads their first 10) and connected set (GetConnectedKeyFrames), maps with their bad flag, and
 * frames (mnId and BowVector) for relocalisation.  Word ids ascend inside a vector and lie below n_words. */
typedef struct osh_host_kfdb_graph {
  int64_t n_words;
  int32_t n_kf;
  const int32_t* kf_id;      /* [n_kf]   mnId                                         */
  const int32_t* kf_map;     /* [n_kf]   index of its map                             */
  const uint8_t* kf_bad;     /* [n_kf]   isBad()                                      */
  const int32_t* bow_start;  /* [n_kf+1] mBowVec of keyframe k: entries [bow_start[k], bow_start[k+1]) */
  const int32_t* bow_word;
  const double* bow_value;
  const int32_t* cov_start;  /* [n_kf+1] mvpOrderedConnectedKeyFrames, as keyframe indices */
  const int32_t* cov;
  const int32_t* con_start;  /* [n_kf+1] keys of mConnectedKeyFrameWeights             */
  const int32_t* con;
  int32_t n_maps;
  const uint8_t* map_bad;    /* [n_maps] Map::IsBad()                                 */
  int32_t n_frames;
  const int32_t* fr_id;      /* [n_frames] mnId                                       */
  const int32_t* fr_start;   /* [n_frames+1]                                          */
  const int32_t* fr_word;
  const double* fr_value;
} osh_host_kfdb_graph;
/* A script is n_ops triples (code, a, b). */
#define OSH_HOST_KFDB_ADD        0  /* add(keyframe a)                                                    */
#define OSH_HOST_KFDB_ERASE      1  /* erase(keyframe a)                                                  */
#define OSH_HOST_KFDB_CLEAR_MAP  2  /* clearMap(map a)                                                    */
#define OSH_HOST_KFDB_CLEAR      3  /* clear()                                                            */
#define OSH_HOST_KFDB_NBEST      4  /* DetectNBestCandidates(keyframe a, loop, merge, b)                  */
#define OSH_HOST_KFDB_RELOC      5  /* DetectRelocalizationCandidates(frame a, map b); result in `loop`   */
/* Per query of the script, in script order (each pointer may be NULL): the candidate lists as keyframe indices and, after the query,
 * of every keyframe mnPlaceRecognitionQuery, mnPlaceRecognitionWords, mnRelocQuery, mnRelocWords (marker) and
 * mPlaceRecognitionScore, mRelocScore (score). */
typedef struct osh_host_kfdb_out {
  int32_t* n_loop;   /* [queries]          */
  int32_t* loop;     /* [queries * n_kf]   */
  int32_t* n_merge;  /* [queries]          */
  int32_t* merge;    /* [queries * n_kf]   */
  int64_t* marker;   /* [queries * n_kf * 4] */
  float* score;      /* [queries * n_kf * 2] */
} osh_host_kfdb_out;
/* The script on a plain single-thread restatement of the reference's class with its std::vector<std::list<KeyFrame*>> inverted file
 * (the bad-keyframe skip at :712 as in the drop-in class).  Returns the number of queries, -1 for bad arguments.  *ms = wall time
 * of the queries alone. */
int osh_host_kfdb_restatement(const osh_host_kfdb_graph* graph, int32_t n_ops, const int32_t* ops, const osh_host_kfdb_out* out, double* ms);
/* The script on an ORB_SLAM3::KeyFrameDatabase constructed on the vocabulary.  -2: the vocabulary has fewer than n_words words. */
int osh_host_kfdb_run(osh_host_bow_vocab* voc, const osh_host_kfdb_graph* graph, int32_t n_ops, const int32_t* ops, const osh_host_kfdb_out* out,
                      double* ms);
/* bowdb_check_words of csrc/bowdb_book.h: 0 accepted, 1 not ascending or a duplicate, 2 an id outside [0, n_words). */
int osh_host_bowdb_check_words(int32_t n, const int32_t* word_id, int64_t n_words);
/* A script of n_ops pairs (0, entries of the new row) / (1, handle to erase) / (2, unused: clear) through BowDbBook of
 * csrc/bowdb_book.h the way osh_bow_db runs it; needs no device.  op_handle [n_ops]: the handle an add returned (0 otherwise).
 * The row table afterwards (up to max_rows rows; each array may be NULL) and info = live rows, rows, entries, entry capacity,
 * compactions, reallocations, row capacity, entries moved by the plans.  Returns the rows of the table; -1 bad arguments, -2 an
 * erase of a handle that names no live row, -3 more than max_rows rows. */
int osh_host_bowdb_book_replay(int32_t n_ops, const int64_t* ops, uint64_t* op_handle, int32_t max_rows, uint64_t* handle, int64_t* start,
                               int32_t* len, uint8_t* alive, int64_t info[8]);

/* ---- MapPoint::RefreshBatch, LocalMapping::SearchInNeighbors / ProcessNewKeyFrame (include/MapPoint.h, include/LocalMapping.h,
 *      csrc/host/MapPoint.cc, csrc/host/LocalMapping.cc, csrc/hosttest/mappoints.cc) ---- */
struct osh_mappoint_batch;
struct osh_mappoint_result;
/* csrc/mappoint_refresh.h (the statements k_mappoint_wave / k_mappoint_block run) compiled for the host, on one thread: arguments as
 * osh_orb_refresh_map_points without a context, without its validation (the batches must be valid) and without its limit on the
 * entries of a point.  *ms (may be NULL) = wall time of the loops over the points.  -1: bad arguments. */
int osh_host_mappoint_refresh_cpu(int32_t n_batches, const struct osh_mappoint_batch* batches, const struct osh_mappoint_result* results,
                                  double* ms);
/* Makes the keyframes of a graph fit for ORBmatcher::Fuse and MapPoint::RefreshBatch: the level tables scale_factor^level by
 * repeated float multiplication (n_levels of them), mfLogScaleFactor, invfx / invfy, mb, mvKeys = mvKeysUn, N, the image bounds
 * (min x, min y, max x, max y) and the grid of the left / only camera, and mDescriptors: kf_rows[k] rows for keyframe k (it must
 * be the length of its match table: left keypoints, then the right ones of a rig), all keyframes one after another in desc.
 * -1: bad arguments. */
int osh_host_graph_set_mapping(osh_host_graph* g, float scale_factor, int32_t n_levels, const float bounds[4], float mb,
                               const int32_t* kf_rows, const uint8_t* desc);
/* mpRefKF of n points (kf[i] = -1: none). */
int osh_host_graph_set_ref_kf(osh_host_graph* g, int32_t n, const int32_t* mp, const int32_t* kf);
/* Takes the observation of keyframe kf out of point mp: the keypoint stays.  keep_match: the keyframe's slot keeps the point (a
 * keyframe fresh from Tracking, whose points do not know it yet); else the slot is emptied.  No bad flag, no new reference. */
int osh_host_graph_unlink(osh_host_graph* g, int32_t kf, int32_t mp, int32_t keep_match);
/* A second map point (id new_id) at the position of point mp that takes over its observations in the n_kf keyframes listed: the
 * duplicate a fusion finds.  Returns the index of the new point; -1: bad arguments. */
int osh_host_graph_clone_point(osh_host_graph* g, int32_t mp, int64_t new_id, int32_t n_kf, const int32_t* kf);
/* MapPoint::RefreshBatch on the points mp[0..n) in that order (-1: a null entry). */
int osh_host_mp_refresh_batch(osh_host_graph* g, int32_t n, const int32_t* mp);
/* What RefreshBatch packs for that list (PackMapPointRefresh of csrc/host/host_pack.h), without a device: sizes = points,
 * entries, centres; every array may be NULL (call once for the sizes).  point_mp: the point of each packed occurrence; entry_kf /
 * entry_row: the keyframe and descriptor row of each entry; the others as osh_mappoint_batch. */
int osh_host_mp_refresh_pack(osh_host_graph* g, int32_t n, const int32_t* mp, int32_t sizes[3], int32_t* point_mp, int32_t* entry_off,
                             int32_t* entry_kf, int32_t* entry_row, uint8_t* desc, int32_t* centre, uint8_t* use_desc, float* centres,
                             float* pos, int32_t* ref_centre, float* level_scale, float* top_scale);
/* mDescriptor (zeros when empty), mNormalVector, mfMinDistance / mfMaxDistance and the counters mnDescriptorUpdates /
 * mnNormalUpdates of a point.  Returns 1 when the point has a descriptor, 0 when not, -1: bad arguments. */
int osh_host_mp_get_refresh(osh_host_graph* g, int32_t mp, uint8_t desc[32], float normal[3], float min_max[2], int32_t counts[2]);
/* The observations of a point in the order std::map<KeyFrame*, ...> iterates (by pointer value; the order both reference functions
 * walk): keyframe index, left index, right index.  Returns their number (which may exceed capacity). */
int osh_host_mp_observations(osh_host_graph* g, int32_t mp, int32_t capacity, int32_t* kf, int32_t* left, int32_t* right);
/* out = isBad, GetReplaced as a point index (-1: none), mnFuseCandidateForKF, the reference keyframe's index (-1: none). */
int osh_host_mp_state(osh_host_graph* g, int32_t mp, int64_t out[4]);
/* GetMapPointMatches of a keyframe as point indices (-1: empty slot).  Returns its length. */
int osh_host_kf_matches(osh_host_graph* g, int32_t kf, int32_t capacity, int32_t* mp);
/* marks = mnFuseTargetForKF, the calls of UpdateConnections, NLeft; centres = GetCameraCenter, GetRightCameraCenter (the left one
 * again without a rig).  Each may be NULL. */
int osh_host_kf_state(osh_host_graph* g, int32_t kf, int64_t marks[3], float centres[6]);
/* One ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th, bRight) on the graph; returns its result. */
int osh_host_graph_fuse(osh_host_graph* g, int32_t kf, int32_t n, const int32_t* mp, float th, int32_t right);
/* LocalMapping::SearchInNeighbors with mpCurrentKeyFrame = keyframe kf and the three flags. */
int osh_host_local_mapping_search_in_neighbors(osh_host_graph* g, int32_t kf, int32_t monocular, int32_t inertial, int32_t abort_ba);
/* LocalMapping::ProcessNewKeyFrame with keyframe kf alone in mlNewKeyFrames (its BoW vectors are marked as computed).  Returns the
 * length of mlpRecentAddedMapPoints, the first `capacity` as point indices in recent; *in_map = how many times more the map lists
 * the keyframe than before. */
int osh_host_local_mapping_process_new_keyframe(osh_host_graph* g, int32_t kf, int32_t capacity, int32_t* recent, int32_t* in_map);

/* ---- LocalMapping::KeyFrameCulling and MapPointCulling (csrc/hosttest/kfcull.cc) ---- */
/* A stand-in map for the two culling steps.  Keyframe i has kf_n_slots[i] slots (its keypoints and match table), the first
 * kf_n_left[i] of them left keypoints of a rig (-1: no rig, all in mvKeysUn); kf_camera2: mpCamera2 is set.  The slots of all
 * keyframes follow one another: the point held (-1: none; it gets the observation through MapPoint::AddObservation), the
 * keypoint's octave, mvuRight and mvDepth.  mp_n_obs overrides the point's nObs where it is not -1. */
typedef struct osh_host_cull_scene {
  int32_t n_kf;
  const int64_t* kf_id;
  const int32_t* kf_n_slots;
  const int32_t* kf_n_left;
  const uint8_t* kf_camera2;
  const float* kf_th_depth;
  const double* kf_timestamp;
  const uint8_t* kf_not_erase;
  const uint8_t* kf_bad;
  const float* kf_imu_pos;      /* [n_kf*3] GetImuPosition() */
  const int32_t* kf_prev;       /* mPrevKF / mNextKF as keyframe indices, -1: none */
  const int32_t* kf_next;
  const uint8_t* kf_has_preint; /* the keyframe owns an IMU::Preintegrated */
  const int32_t* slot_point;
  const int32_t* slot_octave;
  const float* slot_u_right;
  const float* slot_depth;
  int32_t n_mp;
  const int32_t* mp_n_obs;
  const uint8_t* mp_bad;
  int64_t init_kf_id;           /* Map::GetInitKFid() */
  int32_t keyframes_in_map;     /* Map::KeyFramesInMap() */
  int32_t imu_initialized;      /* Map::isImuInitialized() */
  int32_t inertial_ba2;         /* Map::GetIniertialBA2() */
} osh_host_cull_scene;
osh_host_graph* osh_host_cull_graph_create(const osh_host_cull_scene* scene);   /* NULL: bad arguments; freed by osh_host_graph_destroy */
/* LocalMapping::KeyFrameCulling with mpCurrentKeyFrame = keyframe kf (its covisibility list: osh_host_graph_set_covisible) and
 * the three flags.  Returns the number of keyframes the call made bad, the first `capacity` of them in list order in culled;
 * *n_device_calls = the osh_orb_keyframe_cull_count calls it made (0 on the host path).  After the call the wrapper evaluates the
 * state rule of csrc/keyframe_cull.h for every packed point under the set of culled keyframes and compares it with the objects
 * (Observations(), isBad()): -2 when they differ.  -1: bad arguments. */
int osh_host_local_mapping_keyframe_culling(osh_host_graph* g, int32_t kf, int32_t monocular, int32_t inertial, int32_t abort_ba,
                                            int32_t capacity, int32_t* culled, int32_t* n_device_calls);
/* LocalMapping::MapPointCulling with mpCurrentKeyFrame = keyframe kf and mlpRecentAddedMapPoints = the points mp[0..n).  Returns the
 * length of the list afterwards, the first `capacity` as point indices in remaining. */
int osh_host_local_mapping_map_point_culling(osh_host_graph* g, int32_t kf, int32_t monocular, int32_t n, const int32_t* mp,
                                             int32_t capacity, int32_t* remaining);
/* mnFirstKFid, mnVisible and mnFound of a point (what MapPointCulling reads). */
int osh_host_mp_set_culling(osh_host_graph* g, int32_t mp, int64_t first_kf_id, int32_t n_visible, int32_t n_found);
/* What KeyFrameCulling packs for the candidate list kf[0..n) (PackKeyFrameCull of csrc/host/host_pack.h), without a device:
 * sizes = table entries, slots, points, observations; every array may be NULL (call once for the sizes).  table_kf: the keyframe
 * of each table entry; slot_point and obs_kf index the packed points and the table; slot_index: the slot's place in its keyframe;
 * point_mp: the map point of each packed point; the others as osh_kfcull_problem. */
int osh_host_kfcull_pack(osh_host_graph* g, int32_t n, const int32_t* kf, int32_t monocular, int32_t sizes[4], int32_t* table_kf,
                         int32_t* cand_slot_off, int32_t* slot_point, int32_t* slot_level, int32_t* slot_index, int32_t* point_mp,
                         int32_t* point_n_obs, uint8_t* point_bad, int32_t* point_obs_off, int32_t* obs_kf, int32_t* obs_level,
                         int32_t* obs_weight);
/* csrc/keyframe_cull.h on the host in one thread: the results of osh_orb_keyframe_cull_count for a valid problem (it is not
 * validated here); *ms = the wall time of the counting loop. */
struct osh_kfcull_problem;
struct osh_kfcull_result;
int osh_host_keyframe_cull_cpu(const struct osh_kfcull_problem* problem, int32_t n_removed, const int32_t* removed_kf,
                               int32_t first_candidate, const struct osh_kfcull_result* result, double* ms);
/* For profiles/keyframe_cull_timing.py, on the candidate list kf[0..n): ms[0] = the wall time of PackKeyFrameCull; ms[1] = that of
 * the counting loop in the reference's shape on the same objects in one thread (per candidate and slot a copy of GetObservations()
 * and a walk over it); totals = the sums of nMPs and nRedundantObservations that loop finds. */
int osh_host_kfcull_time(osh_host_graph* g, int32_t n, const int32_t* kf, int32_t monocular, double ms[2], int64_t totals[2]);
/* out = isBad, mbToBeErased, mPrevKF, mNextKF (keyframe indices, -1: none), the calls of UpdateBestCovisibles, the connection and
 * the spanning-tree updates SetBadFlag counted, the keyframe whose preintegration this one's MergePrevious received last (-1:
 * none), the number of MergePrevious calls. */
int osh_host_kf_cull_state(osh_host_graph* g, int32_t kf, int64_t out[9]);
/* out = Observations(), isBad(), the size of GetObservations(). */
int osh_host_mp_cull_state(osh_host_graph* g, int32_t mp, int64_t out[3]);

/* ---- ORBmatcher::Fuse for many targets (csrc/orb_fuse.h, csrc/hosttest/fuse_batch.cc) ---- */
struct osh_fuse_target;
struct osh_fuse_points;
struct osh_fuse_result;
/* csrc/orb_fuse.h (the statements k_fuse_project / k_fuse_search run) compiled for the host, on one thread, the grids binned by
 * csrc/orb_grid_bin.h: arguments and results as osh_orb_fuse_search without a context and without its validation (the call must be
 * valid).  *ms (may be NULL) = wall time of the whole call.  -1: bad arguments or a cell above OSH_FUSE_MAX_CELL_ENTRIES. */
int osh_host_fuse_search_cpu(int32_t n_targets, const struct osh_fuse_target* targets, const struct osh_fuse_points* points, int32_t mode,
                             const struct osh_fuse_result* result, double* ms);
/* MapPoint::sbRecomputeDescriptors of the stand-in: when on, MapPoint::ComputeDistinctiveDescriptors (and with it MapPoint::Replace)
 * really picks the descriptor, as the reference does; off by default, process wide. */
void osh_host_set_recompute_descriptors(int32_t on);
/* ORBmatcher::FuseBatch(targets, vpMapPoints) on the graph: target k = (keyframe kf[k], th[k], right[k]); mp: the list (-1: a null
 * entry).  cpu_search: the search runs by csrc/orb_fuse.h on the calling thread instead of the device.  fused [n_targets]: the
 * returned counts; researched [2] = mnFuseBatchResearched, mnFuseBatchResearchedChanged.  -1: bad arguments. */
int osh_host_graph_fuse_batch(osh_host_graph* g, int32_t n_targets, const int32_t* kf, const float* th, const uint8_t* right, int32_t n,
                              const int32_t* mp, int32_t cpu_search, int32_t* fused, int32_t* researched);
/* The Sim3 overload of FuseBatch: sim3 [n_targets*8] = qw qx qy qz tx ty tz s of every Scw.  replace_after: `after(k)` runs
 * LoopClosing::SearchAndFuse's loop, vpReplacePoints[i]->Replace(vpPoints[i]).  replace [n_targets*n] (may be NULL): every
 * vpReplacePoint list as point indices (-1: none). */
int osh_host_graph_fuse_batch_sim3(osh_host_graph* g, int32_t n_targets, const int32_t* kf, const float* sim3, int32_t n, const int32_t* mp,
                                   float th, int32_t cpu_search, int32_t replace_after, int32_t* fused, int32_t* replace, int32_t* researched);
/* One ORBmatcher::Fuse(KeyFrame*, Sim3f&, vpPoints, th, vpReplacePoint) on the graph; returns its result, replace [n] as above. */
int osh_host_graph_fuse_sim3(osh_host_graph* g, int32_t kf, const float sim3[8], int32_t n, const int32_t* mp, float th, int32_t* replace);
/* point mp ->Replace(point by). */
int osh_host_graph_replace(osh_host_graph* g, int32_t mp, int32_t by);
/* LoopClosing::SearchAndFuse: with_poses: the KeyFrameAndPose overload, sim3 [n_kf*8] doubles (qw qx qy qz tx ty tz s) of the g2o::Sim3
 * of every keyframe; else the keyframe-list overload.  order [n_kf]: the keyframe indices in the order the call walked them (the
 * map's order is by pointer value).  info = replacements made, mnFuseBatchResearched, mnFuseBatchResearchedChanged. */
int osh_host_loop_search_and_fuse(osh_host_graph* g, int32_t with_poses, int32_t n_kf, const int32_t* kf, const double* sim3, int32_t n,
                                  const int32_t* mp, int32_t cpu_search, int32_t* order, int32_t info[3]);
/* What one ORBmatcher::Fuse call decides per point before its device search (FuseCandidateLists of csrc/host/ORBmatcher.cc: the
 * stand-in camera's own project, the SE3f pose, KeyFrame::GetFeaturesInArea): sim3 NULL: the first overload with (th, right); else
 * the Sim3 overload through that Scw (8 floats).  count [n]: the length of the point's candidate list, -1 when the point is no
 * query; cand: the lists one after another as indices in the keyframe's own arrays, the first `capacity` of them.  Returns the
 * total length of the lists; -1: bad arguments. */
int osh_host_graph_fuse_candidates(osh_host_graph* g, int32_t kf, const float* sim3, float th, int32_t right, int32_t n, const int32_t* mp,
                                   int32_t* count, int32_t capacity, int32_t* cand);
/* The same call as FuseBatch sees it: the pack of that one target (csrc/host/fuse_batch.h) searched by csrc/orb_fuse.h on the calling
 * thread (cpu_search) or by osh_orb_fuse_search.  stage, n_candidates, best_idx (in the keyframe's own arrays), best_dist [n].
 * -1: bad arguments, -2: the search failed. */
int osh_host_graph_fuse_pack_search(osh_host_graph* g, int32_t kf, const float* sim3, float th, int32_t right, int32_t n, const int32_t* mp,
                                    int32_t cpu_search, int32_t* stage, int32_t* n_candidates, int32_t* best_idx, int32_t* best_dist);

#ifdef __cplusplus
}
#endif
#endif
