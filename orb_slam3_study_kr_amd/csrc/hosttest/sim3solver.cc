// sim3solver.cc -- the C wrappers of include/orbslam3_hip_host.h for the Sim3 RANSAC of loop closing: osh_host_sim3r_cpu runs the
// host build of csrc/sim3_ransac.h (s3r_solve_host, the statements of sim3_ransac_device.hip on one thread; the CPU side of
// tests/test_sim3_ransac_cpu.py and of profiles/sim3_ransac_timing.py), the others expose its stages and the drop-in class
// (include/Sim3Solver.h) on the stand-in classes.  Test library only.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../sim3_ransac.h"
#include "CameraModels/GeometricCamera.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Sim3Solver.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

using ORB_SLAM3::Sim3Solver;

namespace {
// A Sim3Solver of the stand-in classes with what its constructor reads kept alive beside it
struct Sim3Box {
  std::vector<std::unique_ptr<ORB_SLAM3::GeometricCamera> > cameras;
  std::vector<std::unique_ptr<ORB_SLAM3::KeyFrame> > keyframes;
  std::vector<std::unique_ptr<ORB_SLAM3::MapPoint> > points;
  std::unique_ptr<Sim3Solver> solver;
  Sim3Solver::Round round;
};
Sim3Box* box(void* h) { return static_cast<Sim3Box*>(h); }
}  // namespace

extern "C" int osh_host_sim3r_cpu(int32_t n_problems, const osh_sim3r_problem* problems, const osh_sim3r_result* results, double* ms) {
  if (n_problems < 0 || (n_problems && (!problems || !results))) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_problems; ++k) {
    if (problems[k].n < 0 || problems[k].n_iterations < 0) return -1;
    osh::s3r_solve_host(problems[k], results[k]);
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_sim3r_check_inliers(const osh_sim3r_problem* problem, int32_t n_T, const float* T12s, int32_t* count, uint32_t* mask) {
  if (!problem || n_T < 0 || problem->n < 0 || (n_T && (!T12s || !count || !mask))) return -1;
  const size_t words = (size_t)OSH_SIM3R_MASK_WORDS(problem->n);
  for (int k = 0; k < n_T; ++k) count[k] = osh::s3r_check_inliers_host(*problem, T12s + 13 * (size_t)k, mask + words * (size_t)k);
  return 0;
}

extern "C" int osh_host_sim3r_compute_sim3(const float* P1, const float* P2, int32_t fix_scale, float* T13) {
  if (!P1 || !P2 || !T13) return -1;
  osh::s3r_compute_sim3(P1, P2, fix_scale != 0, T13);
  return 0;
}

extern "C" int osh_host_sim3r_scan(int32_t n_iterations, const int32_t* count, int32_t min_inliers, int32_t best_inliers_in, int32_t* record,
                                   int32_t* out) {
  if (n_iterations < 0 || !out || (n_iterations && (!count || !record))) return -1;
  osh::S3rHead H;
  osh::s3r_scan_records(count, n_iterations, min_inliers, best_inliers_in, record, H);
  out[0] = H.first_hit; out[1] = H.n_records; out[2] = H.best_iteration; out[3] = H.best_count;
  return 0;
}

extern "C" int osh_host_sim3r_max_iterations(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations) {
  return osh::s3r_max_iterations(n, probability, min_inliers, max_iterations);
}

extern "C" void* osh_host_sim3_solver_create(const osh_host_sim3_scene* sc) {
  if (!sc || sc->n_kf < 2 || sc->n_kf > 3 || sc->n_levels < 1 || !sc->level_sigma2 || sc->n_points < 0 || sc->n1 < 0) return nullptr;
  if (sc->n_points && (!sc->world || !sc->bad || !sc->index_in_kf)) return nullptr;
  if (sc->n1 && (!sc->kf1_mp || !sc->matched12)) return nullptr;
  for (int k = 0; k < sc->n_kf; ++k) {
    if ((sc->camera_type[k] != 0 && sc->camera_type[k] != 1) || sc->n_keys[k] < 0 || (sc->n_keys[k] && (!sc->xy[k] || !sc->octave[k]))) return nullptr;
    for (int i = 0; i < sc->n_keys[k]; ++i) if (sc->octave[k][i] < 0 || sc->octave[k][i] >= sc->n_levels) return nullptr;
  }
  for (int p = 0; p < sc->n_points; ++p)
    for (int k = 0; k < sc->n_kf; ++k) if (sc->index_in_kf[3 * p + k] >= sc->n_keys[k]) return nullptr;
  for (int i = 0; i < sc->n1; ++i) {
    if (sc->kf1_mp[i] >= sc->n_points || sc->matched12[i] >= sc->n_points) return nullptr;
    if (sc->matched_kf && (sc->matched_kf[i] < 0 || sc->matched_kf[i] >= sc->n_kf)) return nullptr;
  }
  Sim3Box* b = new Sim3Box();
  for (int k = 0; k < sc->n_kf; ++k) {
    if (sc->camera_type[k] == 0) b->cameras.emplace_back(new ORB_SLAM3::Pinhole(std::vector<float>(sc->camera[k], sc->camera[k] + 4)));
    else b->cameras.emplace_back(new ORB_SLAM3::KannalaBrandt8(std::vector<float>(sc->camera[k], sc->camera[k] + 8)));
    b->keyframes.emplace_back(new ORB_SLAM3::KeyFrame((long unsigned)k, nullptr));
    ORB_SLAM3::KeyFrame& kf = *b->keyframes.back();
    kf.mpCamera = b->cameras.back().get();
    for (int i = 0; i < 9; ++i) kf.mRcw.v[i] = sc->Rcw[k][i];   // the entries as given: no trip through a quaternion
    kf.mTcw.set_raw(Eigen::Quaternionf(), Eigen::Vector3f(sc->tcw[k][0], sc->tcw[k][1], sc->tcw[k][2]));
    kf.N = sc->n_keys[k];
    kf.mvKeysUn.resize(sc->n_keys[k]);
    for (int i = 0; i < sc->n_keys[k]; ++i) {
      kf.mvKeysUn[i].pt.x = sc->xy[k][2 * i]; kf.mvKeysUn[i].pt.y = sc->xy[k][2 * i + 1]; kf.mvKeysUn[i].octave = sc->octave[k][i];
    }
    kf.mvKeys = kf.mvKeysUn;
    kf.mvLevelSigma2.assign(sc->level_sigma2, sc->level_sigma2 + sc->n_levels);
    kf.mvpMapPoints.assign(k == 0 ? sc->n1 : sc->n_keys[k], nullptr);
  }
  for (int p = 0; p < sc->n_points; ++p) {
    b->points.emplace_back(new ORB_SLAM3::MapPoint((long unsigned)p, Eigen::Vector3f(sc->world[3 * p], sc->world[3 * p + 1], sc->world[3 * p + 2]), nullptr));
    ORB_SLAM3::MapPoint& mp = *b->points.back();
    mp.mbBad = sc->bad[p] != 0;
    for (int k = 0; k < sc->n_kf; ++k)
      if (sc->index_in_kf[3 * p + k] >= 0) mp.mObservations[b->keyframes[k].get()] = std::tuple<int, int>(sc->index_in_kf[3 * p + k], -1);
  }
  std::vector<ORB_SLAM3::MapPoint*> matched(sc->n1, nullptr);
  std::vector<ORB_SLAM3::KeyFrame*> matched_kf;
  for (int i = 0; i < sc->n1; ++i) {
    if (sc->kf1_mp[i] >= 0) b->keyframes[0]->mvpMapPoints[i] = b->points[sc->kf1_mp[i]].get();
    if (sc->matched12[i] >= 0) matched[i] = b->points[sc->matched12[i]].get();
  }
  if (sc->matched_kf) for (int i = 0; i < sc->n1; ++i) matched_kf.push_back(b->keyframes[sc->matched_kf[i]].get());
  b->solver.reset(new Sim3Solver(b->keyframes[0].get(), b->keyframes[1].get(), matched, sc->fix_scale != 0, matched_kf));
  return b;
}

extern "C" void osh_host_sim3_solver_destroy(void* h) { delete box(h); }

extern "C" int osh_host_sim3_solver_set_ransac(void* h, double probability, int32_t min_inliers, int32_t max_iterations) {
  if (!h) return -1;
  box(h)->solver->SetRansacParameters(probability, min_inliers, max_iterations);
  return 0;
}

extern "C" int osh_host_sim3_solver_state(void* h, int32_t* out) {
  if (!h || !out) return -1;
  const Sim3Solver& s = *box(h)->solver;
  out[0] = s.GetN(); out[1] = s.GetN1(); out[2] = s.GetMinInliers(); out[3] = s.GetMaxIterations(); out[4] = s.GetIterations();
  out[5] = s.GetBestInliers(); out[6] = s.HasAnswer() ? 1 : 0; out[7] = s.mbLastOnDevice ? 1 : 0;
  return 0;
}

extern "C" int osh_host_sim3_solver_pack(void* h, float* x3dc1, float* x3dc2, float* p1im1, float* p2im2, float* max_error1, float* max_error2,
                                         int32_t* indices1) {
  if (!h || !x3dc1 || !x3dc2 || !p1im1 || !p2im2 || !max_error1 || !max_error2 || !indices1) return -1;
  const Sim3Solver& s = *box(h)->solver;
  const size_t n = (size_t)s.GetN();
  if (n) {
    std::memcpy(x3dc1, s.GetX3Dc1().data(), n * 12); std::memcpy(x3dc2, s.GetX3Dc2().data(), n * 12);
    std::memcpy(p1im1, s.GetP1im1().data(), n * 8); std::memcpy(p2im2, s.GetP2im2().data(), n * 8);
    std::memcpy(max_error1, s.GetMaxError1().data(), n * 4); std::memcpy(max_error2, s.GetMaxError2().data(), n * 4);
  }
  for (size_t i = 0; i < n; ++i) indices1[i] = (int32_t)s.GetIndices1()[i];
  return 0;
}

extern "C" int osh_host_sim3_solver_best(void* h, float* T12, float* R, float* t, float* scale, uint8_t* flags) {
  if (!h || !T12 || !R || !t || !scale || !flags) return -1;
  Sim3Solver& s = *box(h)->solver;
  const Eigen::Matrix4f T = s.GetEstimatedTransformation();
  const Eigen::Matrix3f r = s.GetEstimatedRotation();
  const Eigen::Vector3f tr = s.GetEstimatedTranslation();
  for (int i = 0; i < 16; ++i) T12[i] = T.v[i];
  for (int i = 0; i < 9; ++i) R[i] = r.v[i];
  for (int i = 0; i < 3; ++i) t[i] = tr.v[i];
  *scale = s.GetEstimatedScale();
  const std::vector<bool>& f = s.GetBestInlierFlags();
  for (int i = 0; i < s.GetN(); ++i) flags[i] = i < (int)f.size() && f[i];
  return 0;
}

namespace {
void write_row(int k, int n1, const std::vector<bool>& in, bool noMore, int n, bool converge, const Eigen::Matrix4f& T, uint8_t* no_more,
               int32_t* n_inliers, uint8_t* converged, uint8_t* inliers, float* Tout) {
  no_more[k] = noMore; n_inliers[k] = n; converged[k] = converge;
  // vbInliers as iterate left it (always mN1 entries), cut to n1
  uint8_t* row = inliers + (size_t)k * (size_t)n1;
  std::memset(row, 0, (size_t)n1);
  for (size_t i = 0; i < in.size() && i < (size_t)n1; ++i) row[i] = in[i];
  for (int i = 0; i < 16; ++i) Tout[16 * (size_t)k + i] = T.v[i];
}
}  // namespace

extern "C" int osh_host_sim3_solver_iterate(int32_t n_solvers, void* const* handles, int32_t n_iterations, int32_t mode, int32_t n1,
                                            uint8_t* no_more, int32_t* n_inliers, uint8_t* converged, uint8_t* inliers, float* Tout) {
  if (n_solvers < 0 || n1 < 0 || mode < 0 || mode > 3 || (n_solvers && (!handles || !no_more || !n_inliers || !converged || !inliers || !Tout))) return -1;
  std::vector<Sim3Solver*> solvers(n_solvers);
  for (int k = 0; k < n_solvers; ++k) { if (!handles[k]) return -1; solvers[k] = box(handles[k])->solver.get(); }
  if (mode == 2) {
    std::vector<bool> vbNoMore, vbConverge;
    std::vector<std::vector<bool> > vvbInliers;
    std::vector<int> vnInliers;
    std::vector<Eigen::Matrix4f> vT;
    Sim3Solver::IterateBatch(solvers, n_iterations, vbNoMore, vvbInliers, vnInliers, vbConverge, vT);
    for (int k = 0; k < n_solvers; ++k) write_row(k, n1, vvbInliers[k], vbNoMore[k], vnInliers[k], vbConverge[k], vT[k], no_more, n_inliers, converged, inliers, Tout);
    return 0;
  }
  for (int k = 0; k < n_solvers; ++k) {
    bool noMore = false, converge = false;
    std::vector<bool> in;
    int n = 0;
    Eigen::Matrix4f T;
    if (mode == 0) T = solvers[k]->iterate(n_iterations, noMore, in, n);
    else if (mode == 1) T = solvers[k]->iterate(n_iterations, noMore, in, n, converge);
    else T = solvers[k]->find(in, n);
    write_row(k, n1, in, noMore, n, converge, T, no_more, n_inliers, converged, inliers, Tout);
  }
  return 0;
}

extern "C" int osh_host_sim3_solver_prepare(void* h, int32_t capacity, int32_t* sets) {
  if (!h || capacity < 0 || (capacity && !sets)) return -1;
  Sim3Box* b = box(h);
  b->round = b->solver->Prepare();
  if (!b->round.pending) return 0;
  for (int i = 0; i < b->round.iterations * 3 && i < capacity * 3; ++i) sets[i] = b->round.sets[i];
  return b->round.iterations;
}

extern "C" int osh_host_sim3_solver_keep(void* h, int32_t n_records, const int32_t* record, const int32_t* record_count, const float* record_T,
                                         const uint32_t* record_mask) {
  if (!h || n_records < 0 || (n_records && (!record || !record_count || !record_T || !record_mask))) return -1;
  Sim3Box* b = box(h);
  if (!b->round.pending || n_records > b->round.iterations) return -1;
  const size_t ni = (size_t)b->round.iterations, words = (size_t)OSH_SIM3R_MASK_WORDS(b->solver->GetN()), nr = (size_t)n_records;
  Sim3Solver::Answer a;
  a.n_records = n_records;
  a.record.assign(ni, -1); a.record_count.assign(ni, 0); a.record_T.assign(ni * 13, 0.f); a.record_mask.assign(ni * words, 0u);
  for (size_t q = 0; q < nr; ++q) { a.record[q] = record[q]; a.record_count[q] = record_count[q]; }
  if (nr) { std::memcpy(a.record_T.data(), record_T, nr * 13 * sizeof(float)); if (words) std::memcpy(a.record_mask.data(), record_mask, nr * words * sizeof(uint32_t)); }
  b->solver->Keep(b->round, a);
  b->round = Sim3Solver::Round();
  return 0;
}

extern "C" int osh_host_sim3_solver_replay(void* h, int32_t n_iterations, int32_t five, int32_t n1, uint8_t* no_more, int32_t* n_inliers,
                                           uint8_t* converged, uint8_t* inliers, float* Tout) {
  if (!h || n1 < 0 || !no_more || !n_inliers || !converged || !inliers || !Tout) return -1;
  bool noMore = false, converge = false;
  std::vector<bool> in;
  int n = 0;
  const Eigen::Matrix4f T = box(h)->solver->Replay(n_iterations, five != 0, noMore, in, n, converge);
  write_row(0, n1, in, noMore, n, converge, T, no_more, n_inliers, converged, inliers, Tout);
  return 0;
}
