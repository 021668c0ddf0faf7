// fuse_batch.cc -- osh_host_fuse_search_cpu (include/orbslam3_hip_host.h): csrc/orb_fuse.h, the statements of k_fuse_project /
// k_fuse_search, on the host in one thread with the grids binned by csrc/orb_grid_bin.h (the CPU side of tests/test_fuse_cpu.py,
// tests/test_gpu_fuse.py and profiles/fuse_batch_timing.py); and the wrappers that drive ORBmatcher::FuseBatch, the Sim3 overload of
// ORBmatcher::Fuse, MapPoint::Replace and LoopClosing::SearchAndFuse on a stand-in graph.  Test library only.
#include <chrono>
#include <cstdint>
#include <vector>

#include "../orb_fuse.h"
#include "../orb_grid_bin.h"
#include "LoopClosing.h"
#include "ORBmatcher.h"
#include "fuse_batch.h"
#include "host_graph.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

extern "C" int osh_host_fuse_search_cpu(int32_t n_targets, const osh_fuse_target* targets, const osh_fuse_points* points, int32_t mode,
                                        const osh_fuse_result* result, double* ms) {
  if (n_targets < 0 || !points || points->n < 0 || (n_targets && !targets) || (n_targets && points->n && !result)) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t P = (size_t)points->n;
  std::vector<int> coff, cidx, cell_of, fill;
  for (int t = 0; t < n_targets; ++t) {
    const osh_fuse_target& S = targets[t];
    osh::FuseTarget T;
    osh::fuse_fill_target(S, T);
    coff.assign((size_t)S.cols * S.rows + 1, 0);
    cidx.assign((size_t)(S.n_keys > 0 ? S.n_keys : 1), 0);
    if (osh::bin_keypoints(S.key_xy, S.n_keys, S.grid_min_x, S.grid_min_y, S.cell_w_inv, S.cell_h_inv, S.cols, S.rows, OSH_FUSE_MAX_CELL_ENTRIES,
                           coff.data(), cidx.data(), cell_of, fill) > OSH_FUSE_MAX_CELL_ENTRIES) return -1;
    const osh::FuseKeys keys = {S.key_xy, S.key_octave, S.key_uright, reinterpret_cast<const uint32_t*>(S.descriptors), coff.data(), cidx.data()};
    for (size_t p = 0; p < P; ++p) {
      const size_t pair = (size_t)t * P + p;
      osh::FuseGeom g;
      osh::fuse_project(T, points->pos + 3 * p, points->normal + 3 * p, points->min_dist[p], points->max_dist[p], points->skip && points->skip[p], g);
      osh::FuseFound f = {0, 0, -1, 256};
      if (g.stage == OSH_FUSE_SEARCHED) {
        f = osh::fuse_scan(T, keys, g, reinterpret_cast<const uint32_t*>(points->desc) + 8 * p, mode);
        if (f.n_in == 0) g.stage = OSH_FUSE_EMPTY;
      }
      if (result->stage) result->stage[pair] = g.stage;
      if (result->u) result->u[pair] = g.u;
      if (result->v) result->v[pair] = g.v;
      if (result->ur) result->ur[pair] = g.ur;
      if (result->level) result->level[pair] = g.level;
      if (result->radius) result->radius[pair] = g.radius;
      if (result->n_candidates) result->n_candidates[pair] = f.n_candidates;
      if (result->best_idx) result->best_idx[pair] = f.best_idx;
      if (result->best_dist) result->best_dist[pair] = f.best_dist;
    }
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

namespace {

bool kf_ok(osh_host_graph* g, int32_t k) { return g && k >= 0 && k < (int)g->kfs.size(); }
bool mp_ok(osh_host_graph* g, int32_t j) { return g && j >= 0 && j < (int)g->mps.size(); }
int mp_index(osh_host_graph* g, MapPoint* pMP) {
  for (size_t j = 0; j < g->mps.size(); ++j) if (g->mps[j].get() == pMP) return (int)j;
  return -1;
}
int kf_index(osh_host_graph* g, KeyFrame* pKF) {
  for (size_t k = 0; k < g->kfs.size(); ++k) if (g->kfs[k].get() == pKF) return (int)k;
  return -1;
}
bool point_list(osh_host_graph* g, int32_t n, const int32_t* mp, std::vector<MapPoint*>& out) {   // -1 is a null entry
  if (!g || n < 0 || (n && !mp)) return false;
  for (int i = 0; i < n; ++i) {
    if (mp[i] != -1 && !mp_ok(g, mp[i])) return false;
    out.push_back(mp[i] < 0 ? nullptr : g->mps[mp[i]].get());
  }
  return true;
}
// qw qx qy qz tx ty tz s
Sophus::Sim3f sim3_of(const float* s) { return Sophus::Sim3f(Eigen::Quaternionf(s[0], s[1], s[2], s[3]), Eigen::Vector3f(s[4], s[5], s[6]), s[7]); }

}  // namespace

extern "C" void osh_host_set_recompute_descriptors(int32_t on) { MapPoint::sbRecomputeDescriptors = on != 0; }

extern "C" int osh_host_graph_fuse_batch(osh_host_graph* g, int32_t n_targets, const int32_t* kf, const float* th, const uint8_t* right, int32_t n,
                                         const int32_t* mp, int32_t cpu_search, int32_t* fused, int32_t* researched) {
  std::vector<MapPoint*> list;
  if (n_targets < 0 || (n_targets && (!kf || !th || !right || !fused)) || !point_list(g, n, mp, list)) return -1;
  std::vector<ORBmatcher::FuseTarget> targets;
  for (int k = 0; k < n_targets; ++k) {
    if (!kf_ok(g, kf[k])) return -1;
    targets.push_back(ORBmatcher::FuseTarget{g->kfs[kf[k]].get(), th[k], right[k] != 0});
  }
  ORBmatcher matcher;
  matcher.mbFuseBatchSearchOnHost = cpu_search != 0;
  const std::vector<int> out = matcher.FuseBatch(targets, list);
  for (int k = 0; k < n_targets; ++k) fused[k] = out[k];
  if (researched) { researched[0] = matcher.mnFuseBatchResearched; researched[1] = matcher.mnFuseBatchResearchedChanged; }
  return 0;
}

extern "C" int osh_host_graph_fuse_batch_sim3(osh_host_graph* g, int32_t n_targets, const int32_t* kf, const float* sim3, int32_t n, const int32_t* mp,
                                              float th, int32_t cpu_search, int32_t replace_after, int32_t* fused, int32_t* replace, int32_t* researched) {
  std::vector<MapPoint*> list;
  if (n_targets < 0 || (n_targets && (!kf || !sim3 || !fused)) || !point_list(g, n, mp, list)) return -1;
  std::vector<std::pair<KeyFrame*, Sophus::Sim3f>> targets;
  for (int k = 0; k < n_targets; ++k) {
    if (!kf_ok(g, kf[k])) return -1;
    targets.push_back(std::make_pair(g->kfs[kf[k]].get(), sim3_of(sim3 + 8 * k)));
  }
  ORBmatcher matcher;
  matcher.mbFuseBatchSearchOnHost = cpu_search != 0;
  std::vector<std::vector<MapPoint*>> vvp;
  ORBmatcher::AfterTarget after;
  if (replace_after) after = [&](int k) { for (int i = 0; i < n; ++i) if (vvp[k][i]) vvp[k][i]->Replace(list[i]); };
  const std::vector<int> out = matcher.FuseBatch(targets, list, th, vvp, after);
  for (int k = 0; k < n_targets; ++k) {
    fused[k] = out[k];
    if (replace) for (int i = 0; i < n; ++i) replace[(size_t)k * n + i] = vvp[k][i] ? mp_index(g, vvp[k][i]) : -1;
  }
  if (researched) { researched[0] = matcher.mnFuseBatchResearched; researched[1] = matcher.mnFuseBatchResearchedChanged; }
  return 0;
}

extern "C" int osh_host_graph_fuse_sim3(osh_host_graph* g, int32_t kf, const float sim3[8], int32_t n, const int32_t* mp, float th, int32_t* replace) {
  std::vector<MapPoint*> list;
  if (!kf_ok(g, kf) || !sim3 || !point_list(g, n, mp, list)) return -1;
  ORBmatcher matcher;
  Sophus::Sim3f Scw = sim3_of(sim3);
  std::vector<MapPoint*> vp(n, static_cast<MapPoint*>(nullptr));
  const int nFused = matcher.Fuse(g->kfs[kf].get(), Scw, list, th, vp);
  if (replace) for (int i = 0; i < n; ++i) replace[i] = vp[i] ? mp_index(g, vp[i]) : -1;
  return nFused;
}

extern "C" int osh_host_graph_replace(osh_host_graph* g, int32_t mp, int32_t by) {
  if (!mp_ok(g, mp) || !mp_ok(g, by)) return -1;
  g->mps[mp]->Replace(g->mps[by].get());
  return 0;
}

extern "C" int osh_host_loop_search_and_fuse(osh_host_graph* g, int32_t with_poses, int32_t n_kf, const int32_t* kf, const double* sim3, int32_t n,
                                             const int32_t* mp, int32_t cpu_search, int32_t* order, int32_t info[3]) {
  std::vector<MapPoint*> list;
  if (n_kf < 0 || (n_kf && !kf) || (with_poses && n_kf && !sim3) || !point_list(g, n, mp, list)) return -1;
  for (int k = 0; k < n_kf; ++k) if (!kf_ok(g, kf[k])) return -1;
  LoopClosing lc;
  lc.mbFuseSearchOnHost = cpu_search != 0;
  if (with_poses) {
    LoopClosing::KeyFrameAndPose poses;
    for (int k = 0; k < n_kf; ++k) {
      const double* s = sim3 + 8 * k;
      poses[g->kfs[kf[k]].get()] = g2o::Sim3(Eigen::Quaterniond(s[0], s[1], s[2], s[3]), Eigen::Vector3d(s[4], s[5], s[6]), s[7]);
    }
    int at = 0;
    if (order) for (const auto& e : poses) order[at++] = kf_index(g, e.first);
    lc.SearchAndFuse(poses, list);
  } else {
    std::vector<KeyFrame*> kfs;
    for (int k = 0; k < n_kf; ++k) { kfs.push_back(g->kfs[kf[k]].get()); if (order) order[k] = kf[k]; }
    lc.SearchAndFuse(kfs, list);
  }
  if (info) { info[0] = lc.mnLastFuseReplaces; info[1] = lc.mnLastFuseResearched; info[2] = lc.mnLastFuseResearchedChanged; }
  return 0;
}

namespace ORB_SLAM3 { osh_orb_ctx* HostMatcherContext(); }   // csrc/host/ORBmatcher.cc

namespace {

// the pose, centre and camera one Fuse call of either overload searches the keyframe through
void fuse_view(KeyFrame* pKF, const float* sim3, bool right, Sophus::SE3f& Tcw, Eigen::Vector3f& Ow, GeometricCamera*& cam) {
  if (sim3) {   // Fuse(KeyFrame*, Sim3f&, ...), csrc/host/ORBmatcher.cc
    const Sophus::Sim3f Scw = sim3_of(sim3);
    const Eigen::Vector3f ts = Scw.translation();
    const float sc = Scw.scale();
    Tcw = Sophus::SE3f(Scw.rotationMatrix(), Eigen::Vector3f(ts(0) / sc, ts(1) / sc, ts(2) / sc));
    Ow = Tcw.inverse().translation(); cam = pKF->mpCamera;
  } else if (right) { Tcw = pKF->GetRightPose(); Ow = pKF->GetRightCameraCenter(); cam = pKF->mpCamera2; }
  else { Tcw = pKF->GetPose(); Ow = pKF->GetCameraCenter(); cam = pKF->mpCamera; }
}

}  // namespace

extern "C" int osh_host_graph_fuse_candidates(osh_host_graph* g, int32_t kf, const float* sim3, float th, int32_t right, int32_t n, const int32_t* mp,
                                              int32_t* count, int32_t capacity, int32_t* cand) {
  std::vector<MapPoint*> list;
  if (!kf_ok(g, kf) || !count || capacity < 0 || (capacity && !cand) || !point_list(g, n, mp, list)) return -1;
  KeyFrame* pKF = g->kfs[kf].get();
  Sophus::SE3f Tcw;
  Eigen::Vector3f Ow;
  GeometricCamera* cam = nullptr;
  fuse_view(pKF, sim3, right != 0, Tcw, Ow, cam);
  std::vector<int> qOf;
  std::vector<uint8_t> qdesc;
  std::vector<int32_t> off, idx;
  FuseCandidateLists(pKF, Tcw, Ow, cam, list, th, right != 0, sim3 == nullptr, qOf, qdesc, off, idx);
  int at = 0;
  for (int i = 0; i < n; ++i) {
    count[i] = qOf[i] < 0 ? -1 : off[qOf[i] + 1] - off[qOf[i]];
    if (qOf[i] >= 0) for (int e = off[qOf[i]]; e < off[qOf[i] + 1]; ++e, ++at) if (at < capacity) cand[at] = idx[e];
  }
  return (int)idx.size();
}

extern "C" int osh_host_graph_fuse_pack_search(osh_host_graph* g, int32_t kf, const float* sim3, float th, int32_t right, int32_t n, const int32_t* mp,
                                               int32_t cpu_search, int32_t* stage, int32_t* n_candidates, int32_t* best_idx, int32_t* best_dist) {
  std::vector<MapPoint*> list;
  if (!kf_ok(g, kf) || !stage || !n_candidates || !best_idx || !best_dist || !point_list(g, n, mp, list)) return -1;
  KeyFrame* pKF = g->kfs[kf].get();
  Sophus::SE3f Tcw;
  Eigen::Vector3f Ow;
  GeometricCamera* cam = nullptr;
  fuse_view(pKF, sim3, right != 0, Tcw, Ow, cam);
  FuseBatchPack pk;
  pk.set_points(list);
  pk.add_target(pKF, Tcw, Ow, cam, th, right != 0, sim3 == nullptr);
  pk.bind();
  FuseBatchFound found;
  found.size((size_t)n);
  const int mode = sim3 ? OSH_FUSE_SIM3 : OSH_FUSE_CHI2;
  if (n) {
    if (cpu_search) { if (!FuseSearchOnHost(pk, mode, found)) return -2; }
    else {
      osh_orb_ctx* ctx = HostMatcherContext();
      if (!ctx || osh_orb_fuse_search(ctx, 1, pk.targets.data(), &pk.points, mode, &found.result) != OSH_OK) return -2;
    }
  }
  for (int i = 0; i < n; ++i) {
    stage[i] = found.stage[i]; n_candidates[i] = found.n_candidates[i]; best_dist[i] = found.best_dist[i];
    best_idx[i] = found.best_idx[i] < 0 ? -1 : found.best_idx[i] + pk.keys[0].row0;
  }
  return 0;
}
