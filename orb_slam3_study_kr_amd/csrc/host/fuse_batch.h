// fuse_batch.h -- ORBmatcher::FuseBatch (csrc/host/ORBmatcher.cc) in three parts: pack (the graph -> osh_fuse_target /
// osh_fuse_points), search (ONE osh_orb_fuse_search, or the same statements of csrc/orb_fuse.h on this thread), replay (the loops of
// the two Fuse overloads, unchanged in order, fed from the batch's results).
//
// The order dependence.  A later target's search reads, of a list point, its position, normal, distance range and descriptor.  What
// an earlier target's replay (or the caller's `after`) does to the map: MapPoint::Replace moves observations and ends in
// ComputeDistinctiveDescriptors() of the surviving point (src/MapPoint.cc:248-297), which can change that point's descriptor;
// AddObservation and KeyFrame::AddMapPoint touch none of the four (src/MapPoint.cc:140-165, src/KeyFrame.cc:297-301), and nothing
// here calls UpdateNormalAndDepth or SetWorldPos.  The stand-ins of include/ and csrc/hosttest/graph_stubs.cc agree: Replace calls
// ComputeDistinctiveDescriptors and nothing else that writes mWorldPos, mNormalVector, mfMinDistance or mfMaxDistance.  So after each
// target's replay and `after`, a list point whose descriptor bytes differ from the uploaded ones is STALE from then on: at a later
// target its geometric results stand and only best_idx / best_dist are redone, by fuse_scan of csrc/orb_fuse.h on this thread with
// the current descriptor.  A point that goes bad needs no rule: the replay's own isBad / IsInKeyFrame / spAlreadyFound checks see it.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../orb_fuse.h"
#include "../orb_grid_bin.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

// The host part of the search inside ORBmatcher::Fuse (csrc/host/ORBmatcher.cc): projection, gates and the explicit candidate lists of
// one keyframe.  qOf[i] = query of point i or -1; query q's candidates are idx[off[q] .. off[q + 1]) in GetFeaturesInArea's order, as
// indices in the keyframe's own arrays; qdesc [32 per query].
void FuseCandidateLists(KeyFrame* pKF, const Sophus::SE3f& Tcw, const Eigen::Vector3f& Ow, GeometricCamera* pCamera, const std::vector<MapPoint*>& vpMapPoints,
                        const float th, const bool bRight, const bool chi2_gate, std::vector<int>& qOf, std::vector<uint8_t>& qdesc,
                        std::vector<int32_t>& off, std::vector<int32_t>& idx);

// ---- pack
struct FuseBatchPack {
  struct Keys { std::vector<float> xy, uright; std::vector<int32_t> octave; int row0 = 0; };   // row0: first descriptor row and slot of the set
  std::vector<osh_fuse_target> targets;
  std::vector<Keys> keys;
  std::vector<float> pos, normal, min_dist, max_dist;
  std::vector<uint8_t> desc, skip;
  osh_fuse_points points{};
  int P = 0;

  void set_points(const std::vector<MapPoint*>& vp) {
    P = (int)vp.size();
    pos.assign(3 * (size_t)P, 0.f); normal.assign(3 * (size_t)P, 0.f); min_dist.assign(P, 0.f); max_dist.assign(P, 0.f);
    desc.assign(32 * (size_t)P, 0); skip.assign(P, 0);
    for (int i = 0; i < P; ++i) {
      MapPoint* pMP = vp[i];
      if (!pMP) { skip[i] = 1; continue; }
      const Eigen::Vector3f p = pMP->GetWorldPos(), n = pMP->GetNormal();
      for (int k = 0; k < 3; ++k) { pos[3 * (size_t)i + k] = p(k); normal[3 * (size_t)i + k] = n(k); }
      min_dist[i] = pMP->mfMinDistance; max_dist[i] = pMP->mfMaxDistance;   // the gates apply 0.8f and 1.2f themselves
      current_descriptor(pMP, &desc[32 * (size_t)i]);
    }
    points.n = P; points.pos = pos.data(); points.normal = normal.data(); points.min_dist = min_dist.data(); points.max_dist = max_dist.data();
    points.desc = desc.data(); points.skip = skip.data();
  }
  static void current_descriptor(MapPoint* pMP, uint8_t out[32]) {
    const cv::Mat d = pMP->GetDescriptor();
    if (d.empty()) std::memset(out, 0, 32); else std::memcpy(out, d.ptr<uint8_t>(0), 32);
  }
  // one target: the keyframe seen through (Tcw, Ow, camera); `own_keys`: the first overload on a rig reads mvKeys / mvKeysRight,
  // everything else mvKeysUn (src/ORBmatcher.cc:1264-1268 against :1420)
  void add_target(KeyFrame* pKF, const Sophus::SE3f& Tcw, const Eigen::Vector3f& Ow, GeometricCamera* cam, float th, bool bRight, bool own_keys) {
    osh_fuse_target t{};
    const Eigen::Matrix3f R = Tcw.rotationMatrix();
    const Eigen::Vector3f tr = Tcw.translation();
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) t.Rcw[3 * r + c] = R(r, c); t.tcw[r] = tr(r); t.Ow[r] = Ow(r); }
    t.camera = cam->GetType() == GeometricCamera::CAM_FISHEYE ? OSH_FUSE_KB8 : OSH_FUSE_PINHOLE;
    t.fx = cam->getParameter(0); t.fy = cam->getParameter(1); t.cx = cam->getParameter(2); t.cy = cam->getParameter(3);
    if (t.camera == OSH_FUSE_KB8) for (int k = 0; k < 4; ++k) t.kb8[k] = cam->getParameter(4 + k);
    t.bf = pKF->mbf;
    t.min_x = (float)pKF->mnMinX; t.max_x = (float)pKF->mnMaxX; t.min_y = (float)pKF->mnMinY; t.max_y = (float)pKF->mnMaxY;
    t.grid_min_x = (float)pKF->mnMinX; t.grid_min_y = (float)pKF->mnMinY;
    t.cell_w_inv = pKF->mfGridElementWidthInv; t.cell_h_inv = pKF->mfGridElementHeightInv; t.cols = pKF->mnGridCols; t.rows = pKF->mnGridRows;
    t.n_levels = pKF->mnScaleLevels; t.log_scale_factor = pKF->mfLogScaleFactor;
    for (int k = 0; k < t.n_levels && k < OSH_FUSE_MAX_LEVELS; ++k) { t.scale_factors[k] = pKF->mvScaleFactors[k]; t.inv_level_sigma2[k] = pKF->mvInvLevelSigma2[k]; }
    t.th = th;
    const bool rig = pKF->NLeft != -1;
    const std::vector<cv::KeyPoint>& kps = (!own_keys || !rig) ? pKF->mvKeysUn : (!bRight) ? pKF->mvKeys : pKF->mvKeysRight;
    Keys k;
    k.row0 = (bRight && rig) ? pKF->NLeft : 0;
    const int n = (int)kps.size();
    k.xy.resize(2 * (size_t)n); k.octave.resize(n); k.uright.resize(n);
    for (int i = 0; i < n; ++i) {
      k.xy[2 * i] = kps[i].pt.x; k.xy[2 * i + 1] = kps[i].pt.y; k.octave[i] = kps[i].octave;
      k.uright[i] = i < (int)pKF->mvuRight.size() ? pKF->mvuRight[i] : -1.f;   // mvuRight[k] with k counted in the searched camera, as the source has it
    }
    t.n_keys = n;
    t.descriptors = n ? pKF->mDescriptors.ptr<uint8_t>(k.row0) : nullptr;
    targets.push_back(t);
    keys.push_back(std::move(k));
  }
  void bind() {   // after the last add_target: the vectors no longer move
    for (size_t k = 0; k < targets.size(); ++k) {
      targets[k].key_xy = keys[k].xy.data(); targets[k].key_octave = keys[k].octave.data(); targets[k].key_uright = keys[k].uright.data();
    }
  }
};

// ---- search
struct FuseBatchFound {
  std::vector<int32_t> stage, level, n_candidates, best_idx, best_dist;
  std::vector<float> u, v, ur, radius;
  osh_fuse_result result{};
  void size(size_t n) {
    for (auto* a : {&stage, &level, &n_candidates, &best_idx, &best_dist}) a->assign(n, 0);
    for (auto* a : {&u, &v, &ur, &radius}) a->assign(n, 0.f);
    result = osh_fuse_result{stage.data(), u.data(), v.data(), ur.data(), level.data(), radius.data(), n_candidates.data(), best_idx.data(), best_dist.data()};
  }
};

// the grid of one packed target, binned by the rule of the upload
struct FuseHostGrid {
  osh::FuseTarget T;
  std::vector<int> coff, cidx;
  osh::FuseKeys keys;
  bool set(const osh_fuse_target& s) {
    osh::fuse_fill_target(s, T);
    coff.assign((size_t)s.cols * s.rows + 1, 0); cidx.assign((size_t)(s.n_keys > 0 ? s.n_keys : 1), 0);
    std::vector<int> cell_of, fill;
    if (osh::bin_keypoints(s.key_xy, s.n_keys, s.grid_min_x, s.grid_min_y, s.cell_w_inv, s.cell_h_inv, s.cols, s.rows, OSH_FUSE_MAX_CELL_ENTRIES, coff.data(),
                           cidx.data(), cell_of, fill) > OSH_FUSE_MAX_CELL_ENTRIES) return false;
    keys = osh::FuseKeys{s.key_xy, s.key_octave, s.key_uright, reinterpret_cast<const uint32_t*>(s.descriptors), coff.data(), cidx.data()};
    return true;
  }
};

// csrc/orb_fuse.h on this thread: what osh_orb_fuse_search computes (the call must be one it would accept)
inline bool FuseSearchOnHost(const FuseBatchPack& pk, int mode, FuseBatchFound& f) {
  const size_t P = (size_t)pk.P;
  FuseHostGrid grid;
  for (size_t t = 0; t < pk.targets.size(); ++t) {
    if (!grid.set(pk.targets[t])) return false;
    for (size_t p = 0; p < P; ++p) {
      const size_t at = t * P + p;
      osh::FuseGeom g;
      osh::fuse_project(grid.T, &pk.pos[3 * p], &pk.normal[3 * p], pk.min_dist[p], pk.max_dist[p], pk.skip[p] != 0, g);
      osh::FuseFound found = {0, 0, -1, 256};
      if (g.stage == OSH_FUSE_SEARCHED) {
        found = osh::fuse_scan(grid.T, grid.keys, g, reinterpret_cast<const uint32_t*>(&pk.desc[32 * p]), mode);
        if (found.n_in == 0) g.stage = OSH_FUSE_EMPTY;
      }
      f.stage[at] = g.stage; f.u[at] = g.u; f.v[at] = g.v; f.ur[at] = g.ur; f.level[at] = g.level; f.radius[at] = g.radius;
      f.n_candidates[at] = found.n_candidates; f.best_idx[at] = found.best_idx; f.best_dist[at] = found.best_dist;
    }
  }
  return true;
}

// ---- replay: the result of (target t, point i) as the sequential loop of Fuse calls would have it
struct FuseBatchReplay {
  const FuseBatchPack& pk;
  const FuseBatchFound& f;
  int mode;
  std::vector<uint8_t> stale;
  int accept;                         // ORBmatcher::TH_LOW
  int researched = 0, changed = 0;   // pairs redone; those whose best index, or whose acceptance (distance <= TH_LOW), came out differently
  FuseHostGrid grid;
  int grid_of = -1;
  FuseBatchReplay(const FuseBatchPack& pack, const FuseBatchFound& found, int m, int th_low) : pk(pack), f(found), mode(m), stale((size_t)pack.P, 0), accept(th_low) {}

  // false: the point is no query of this target (Fuse's qOf[i] < 0).  best is an index in the keyframe's own arrays
  bool best_of(int t, int i, MapPoint* pMP, int& best, int& dist) {
    const size_t at = (size_t)t * pk.P + i;
    if (f.stage[at] != OSH_FUSE_SEARCHED) return false;
    best = f.best_idx[at]; dist = f.best_dist[at];
    if (stale[i]) {
      if (grid_of != t) { grid.set(pk.targets[t]); grid_of = t; }
      uint8_t d[32];
      FuseBatchPack::current_descriptor(pMP, d);
      uint32_t dw[8];
      std::memcpy(dw, d, 32);
      const osh::FuseGeom g{OSH_FUSE_SEARCHED, f.u[at], f.v[at], f.ur[at], f.level[at], f.radius[at]};
      const osh::FuseFound found = osh::fuse_scan(grid.T, grid.keys, g, dw, mode);
      if (found.best_idx != best || (found.best_dist <= accept) != (dist <= accept)) ++changed;
      best = found.best_idx; dist = found.best_dist;
      ++researched;
    }
    if (best >= 0) best += pk.keys[t].row0;
    return true;
  }
  // after a target's replay and `after`: which list points no longer carry the uploaded descriptor
  void mark_stale(const std::vector<MapPoint*>& vp) {
    uint8_t d[32];
    for (int i = 0; i < pk.P; ++i) {
      if (!vp[i] || stale[i]) continue;
      FuseBatchPack::current_descriptor(vp[i], d);
      if (std::memcmp(d, &pk.desc[32 * (size_t)i], 32) != 0) stale[i] = 1;
    }
  }
};

}  // namespace ORB_SLAM3
