// mlpnp.cc -- the C wrappers of include/orbslam3_hip_host.h for the PnP RANSAC of relocalisation: osh_host_mlpnp_cpu runs the host
// build of csrc/mlpnp.h (ml_solve_host, the statements of mlpnp_device.hip on one thread; the CPU side of tests/test_mlpnp_cpu.py and
// of profiles/mlpnp_timing.py), the others expose its stages one by one.  Test library only.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../mlpnp.h"
#include "CameraModels/GeometricCamera.h"
#include "Frame.h"
#include "MLPnPsolver.h"
#include "MapPoint.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

namespace ORB_SLAM3 {

// src/CameraModels/Pinhole.cpp:66-69
cv::Point3f Pinhole::unproject(const cv::Point2f& p2D) {
  return cv::Point3f((p2D.x - mvParameters[2]) / mvParameters[0], (p2D.y - mvParameters[3]) / mvParameters[1], 1.f);
}
// src/CameraModels/KannalaBrandt8.cpp:116-143
cv::Point3f KannalaBrandt8::unproject(const cv::Point2f& p2D) {
  float r[3];
  osh::kb8_unproject(mvParameters.data(), precision, p2D.x, p2D.y, r);
  return cv::Point3f(r[0], r[1], r[2]);
}

}  // namespace ORB_SLAM3

namespace {
// An MLPnPsolver of the stand-in classes with what its constructor reads kept alive beside it
struct SolverBox {
  std::unique_ptr<ORB_SLAM3::GeometricCamera> camera;
  ORB_SLAM3::Frame frame;
  std::vector<std::unique_ptr<ORB_SLAM3::MapPoint> > points;
  std::unique_ptr<ORB_SLAM3::MLPnPsolver> solver;
  ORB_SLAM3::MLPnPsolver::Round round;
};
}  // namespace

extern "C" int osh_host_mlpnp_cpu(int32_t n_problems, const osh_mlpnp_problem* problems, const osh_mlpnp_result* results, double* ms) {
  if (n_problems < 0 || (n_problems && (!problems || !results))) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_problems; ++k) {
    if (problems[k].n < 0 || problems[k].n_iterations < 0 || problems[k].min_inliers < 6) return -1;
    osh::ml_solve_host(problems[k], results[k]);
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_mlpnp_check_inliers(const osh_mlpnp_problem* problem, int32_t n_poses, const double* poses, int32_t* count, uint32_t* mask) {
  if (!problem || n_poses < 0 || problem->n < 0 || (n_poses && (!poses || !count || !mask))) return -1;
  const size_t words = (size_t)OSH_MLPNP_MASK_WORDS(problem->n);
  for (int k = 0; k < n_poses; ++k) count[k] = osh::ml_check_inliers_host(*problem, poses + 12 * (size_t)k, mask + words * (size_t)k);
  return 0;
}

extern "C" int osh_host_mlpnp_nullspace(const double* f, double* N) {
  if (!f || !N) return -1;
  double n[3][2];
  osh::ml_nullspace(f, n);
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 2; ++c) N[2 * r + c] = n[r][c];
  return 0;
}

extern "C" int osh_host_mlpnp_rank(const double* S) {
  if (!S) return -1;
  double s[6];
  for (int r = 0; r < 3; ++r) for (int c = r; c < 3; ++c) s[osh::ml_sym(3, r, c)] = S[3 * r + c];
  return osh::ml_rank3(s);
}

extern "C" int osh_host_mlpnp_null_vector(const double* M, int32_t cols, double* h) {
  if (!M || !h || (cols != 9 && cols != 12)) return -1;
  double a[osh::kMlRows][12];
  for (int i = 0; i < osh::kMlRows; ++i) for (int j = 0; j < 12; ++j) a[i][j] = i < cols && j < cols ? M[cols * i + j] : 0.0;
  double v[12];
  osh::ml_null12(a, cols, v);
  for (int k = 0; k < cols; ++k) h[k] = v[k];
  return 0;
}

extern "C" int osh_host_mlpnp_compute_pose(int32_t n, const double* bearing, const double* p3d, double* pose, int32_t* info) {
  if (n < 6 || !bearing || !p3d || !pose) return -1;
  std::vector<int> idx((size_t)n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  int inf[3] = {0, 0, 0};
  osh::ml_compute_pose_host(n, idx.data(), bearing, p3d, pose, inf);
  if (info) { info[0] = inf[0]; info[1] = inf[1]; info[2] = inf[2]; }
  return 0;
}

extern "C" int osh_host_mlpnp_gauss_newton(int32_t n, const double* bearing, const double* p3d, double* x, int32_t max_iterations, int32_t* info) {
  if (n < 1 || !bearing || !p3d || !x || max_iterations < 0) return -1;
  std::vector<int> idx((size_t)n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  int inf[3] = {0, 0, 0};
  osh::ml_gauss_newton_host(n, idx.data(), bearing, p3d, x, max_iterations, inf);
  if (info) { info[0] = inf[1]; info[1] = inf[2]; }
  return 0;
}

extern "C" int osh_host_mlpnp_replay(int32_t n_iterations, const int32_t* count, int32_t min_inliers, int32_t best_inliers_in, int32_t best_refine_ok_in,
                                     const int32_t* record_count, int32_t* record, int32_t* out) {
  if (n_iterations < 0 || !out || (n_iterations && (!count || !record_count || !record))) return -1;
  osh::MlHead H;
  std::memset(&H, 0, sizeof(H));
  H.n_records = osh::ml_scan_records(count, n_iterations, min_inliers, best_inliers_in, record);
  osh::ml_decide(count, n_iterations, min_inliers, best_inliers_in, best_refine_ok_in, record, record_count, H);
  out[0] = H.first_hit; out[1] = H.hit_record; out[2] = H.hit_count; out[3] = H.best_iteration; out[4] = H.best_count; out[5] = H.best_refine_ok;
  out[6] = H.n_records;
  return 0;
}

extern "C" int osh_host_mlpnp_ransac_parameters(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set, float epsilon,
                                                int32_t* out) {
  if (n < 0 || !out) return -1;
  int a = 0, b = 0;
  osh::ml_ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon, &a, &b);
  out[0] = a; out[1] = b;
  return 0;
}

using ORB_SLAM3::MLPnPsolver;

extern "C" void* osh_host_mlpnp_solver_create(int32_t camera_type, const float* params, int32_t n_keys, const float* xy, const int32_t* octave,
                                              int32_t n_levels, const float* level_sigma2, int32_t n_matches, const float* world,
                                              const uint8_t* state) {
  if ((camera_type != 0 && camera_type != 1) || !params || n_keys < 0 || n_matches < 0 || n_levels < 1 || !level_sigma2) return nullptr;
  if ((n_keys && (!xy || !octave)) || (n_matches && (!world || !state))) return nullptr;
  for (int i = 0; i < n_keys; ++i) if (octave[i] < 0 || octave[i] >= n_levels) return nullptr;
  SolverBox* b = new SolverBox();
  if (camera_type == 0) b->camera.reset(new ORB_SLAM3::Pinhole(std::vector<float>(params, params + 4)));
  else b->camera.reset(new ORB_SLAM3::KannalaBrandt8(std::vector<float>(params, params + 8)));
  b->frame.mpCamera = b->camera.get();
  b->frame.mvKeysUn.resize(n_keys);
  for (int i = 0; i < n_keys; ++i) { b->frame.mvKeysUn[i].pt.x = xy[2 * i]; b->frame.mvKeysUn[i].pt.y = xy[2 * i + 1]; b->frame.mvKeysUn[i].octave = octave[i]; }
  b->frame.mvLevelSigma2.assign(level_sigma2, level_sigma2 + n_levels);
  b->frame.N = n_keys;
  std::vector<ORB_SLAM3::MapPoint*> matches(n_matches, nullptr);
  for (int i = 0; i < n_matches; ++i) {   // state: 0 no map point, 1 a good one, 2 a bad one
    if (!state[i]) continue;
    b->points.emplace_back(new ORB_SLAM3::MapPoint((long unsigned)i, Eigen::Vector3f(world[3 * i], world[3 * i + 1], world[3 * i + 2]), nullptr));
    if (state[i] == 2) b->points.back()->mbBad = true;
    matches[i] = b->points.back().get();
  }
  b->frame.mvpMapPoints = matches;
  b->solver.reset(new MLPnPsolver(b->frame, matches));
  return b;
}

extern "C" void osh_host_mlpnp_solver_destroy(void* h) { delete static_cast<SolverBox*>(h); }

extern "C" int osh_host_mlpnp_solver_set_ransac(void* h, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set,
                                                float epsilon, float th2) {
  if (!h) return -1;
  static_cast<SolverBox*>(h)->solver->SetRansacParameters(probability, min_inliers, max_iterations, min_set, epsilon, th2);
  return 0;
}

extern "C" int osh_host_mlpnp_solver_state(void* h, int32_t* out) {
  if (!h || !out) return -1;
  const MLPnPsolver& s = *static_cast<SolverBox*>(h)->solver;
  out[0] = s.GetN(); out[1] = s.GetMinInliers(); out[2] = s.GetMaxIterations(); out[3] = s.GetIterations(); out[4] = s.GetBestInliers();
  out[5] = (int32_t)s.GetQueuedSets(); out[6] = s.mbLastOnDevice ? 1 : 0;
  return 0;
}

extern "C" int osh_host_mlpnp_solver_iterate(int32_t n_solvers, void* const* handles, int32_t n_iterations, int32_t batch, int32_t n_matches,
                                             uint8_t* found, uint8_t* no_more, int32_t* n_inliers, uint8_t* inliers, float* Tout) {
  if (n_solvers < 0 || n_matches < 0 || (n_solvers && (!handles || !found || !no_more || !n_inliers || !inliers || !Tout))) return -1;
  std::vector<MLPnPsolver*> solvers(n_solvers);
  for (int k = 0; k < n_solvers; ++k) { if (!handles[k]) return -1; solvers[k] = static_cast<SolverBox*>(handles[k])->solver.get(); }
  std::vector<bool> vbFound(n_solvers), vbNoMore(n_solvers);
  std::vector<std::vector<bool> > vvbInliers(n_solvers);
  std::vector<int> vnInliers(n_solvers);
  std::vector<Eigen::Matrix4f> vTout(n_solvers);
  if (batch) MLPnPsolver::IterateBatch(solvers, n_iterations, vbFound, vbNoMore, vvbInliers, vnInliers, vTout);
  else
    for (int k = 0; k < n_solvers; ++k) {
      bool noMore = false, f;
      std::vector<bool> in;
      f = solvers[k]->iterate(n_iterations, noMore, in, vnInliers[k], vTout[k]);
      vbFound[k] = f; vbNoMore[k] = noMore; vvbInliers[k] = in;
    }
  for (int k = 0; k < n_solvers; ++k) {
    found[k] = vbFound[k]; no_more[k] = vbNoMore[k]; n_inliers[k] = vnInliers[k];
    // vbInliers as iterate left it: its size in the last byte of the row's n_matches + 1, its entries before (cut to n_matches)
    uint8_t* row = inliers + (size_t)k * ((size_t)n_matches + 1);
    std::memset(row, 0, (size_t)n_matches + 1);
    for (size_t i = 0; i < vvbInliers[k].size() && i < (size_t)n_matches; ++i) row[i] = vvbInliers[k][i];
    row[n_matches] = vvbInliers[k].empty() ? 0 : 1;
    for (int i = 0; i < 16; ++i) Tout[16 * (size_t)k + i] = vTout[k].v[i];
  }
  return 0;
}

extern "C" int osh_host_mlpnp_solver_prepare(void* h, int32_t n_iterations, int32_t capacity, int32_t* sets) {
  if (!h || capacity < 0 || (capacity && !sets)) return -1;
  SolverBox* b = static_cast<SolverBox*>(h);
  b->round = b->solver->Prepare(n_iterations);
  if (b->round.skip) return -2;
  for (int i = 0; i < b->round.iterations * 6 && i < capacity * 6; ++i) sets[i] = b->round.sets[i];
  return b->round.iterations;
}

extern "C" int osh_host_mlpnp_solver_replay(void* h, const int32_t* head, const double* hit_pose, const uint32_t* hit_mask, const double* best_pose,
                                            const uint32_t* best_mask, int32_t n_matches, uint8_t* no_more, int32_t* n_inliers, uint8_t* inliers,
                                            float* Tout) {
  if (!h || !head || !hit_pose || !hit_mask || !best_pose || !best_mask || n_matches < 0 || !no_more || !n_inliers || !inliers || !Tout) return -1;
  SolverBox* b = static_cast<SolverBox*>(h);
  MLPnPsolver::Outcome o;
  o.first_hit = head[0]; o.hit_record = head[1]; o.hit_count = head[2]; o.best_iteration = head[3]; o.best_count = head[4]; o.best_refine_ok = head[5];
  const size_t words = (size_t)OSH_MLPNP_MASK_WORDS(b->solver->GetN());
  o.hit_mask.assign(hit_mask, hit_mask + words); o.best_mask.assign(best_mask, best_mask + words);
  std::memcpy(o.hit_pose, hit_pose, 96); std::memcpy(o.best_pose, best_pose, 96);
  bool noMore = false;
  std::vector<bool> in;
  int n = 0;
  Eigen::Matrix4f T;
  const bool found = b->solver->Replay(b->round, o, noMore, in, n, T);
  *no_more = noMore; *n_inliers = n;
  std::memset(inliers, 0, (size_t)n_matches + 1);
  for (size_t i = 0; i < in.size() && i < (size_t)n_matches; ++i) inliers[i] = in[i];
  inliers[n_matches] = in.empty() ? 0 : 1;
  for (int i = 0; i < 16; ++i) Tout[i] = T.v[i];
  return found ? 1 : 0;
}
