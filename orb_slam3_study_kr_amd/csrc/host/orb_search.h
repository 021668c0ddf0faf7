// orb_search.h -- the search-and-replay layer the ORBmatcher entry points of csrc/host/ORBmatcher.cc share: the queries and the
// target of one batched device search (windows on the target's grid, or explicit candidate lists), the best / second-best result
// of a query, the reference's own candidate scan for a query whose result was overtaken by an earlier match of the same call,
// the rotation histogram, the walk over two feature vectors and the scale gates of a projected map point.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // the calling thread's matcher context (ORBmatcher.cc); nullptr, after a message, if there is none

// src/ORBmatcher.cc:2058-2074: 8 x 32-bit popcount of a XOR b
inline int hamming256(const uint32_t* a, const uint32_t* b) {
  int dist = 0;
  for (int i = 0; i < 8; ++i) dist += __builtin_popcount(a[i] ^ b[i]);
  return dist;
}

inline void push_desc(std::vector<uint8_t>& out, const cv::Mat& desc, int row) {
  const uint8_t* dp = desc.ptr<uint8_t>(row);
  out.insert(out.end(), dp, dp + 32);
}

// ---- keypoint of a feature index: undistorted (no second camera), else left / right camera of a fisheye stereo layout
inline const cv::KeyPoint& keypoint_of(const Frame& F, int i) {
  return (F.Nleft == -1) ? F.mvKeysUn[i] : (i < F.Nleft) ? F.mvKeys[i] : F.mvKeysRight[i - F.Nleft];
}
inline const cv::KeyPoint& keypoint_of(const KeyFrame* pKF, int i) {
  return (pKF->NLeft == -1) ? pKF->mvKeysUn[i] : (i < pKF->NLeft) ? pKF->mvKeys[i] : pKF->mvKeysRight[i - pKF->NLeft];
}

// ---- best and second-best candidate of one query, updated the way every candidate loop of the reference does it
struct Best2 {
  int idx = -1, dist = 256, dist2 = 256, level = -1, level2 = -1;
  void offer(int i, int d, int lvl) {
    if (d < dist) { dist2 = dist; dist = d; level2 = level; level = lvl; idx = i; }
    else if (d < dist2) { level2 = lvl; dist2 = d; }
  }
};

// what the device found for every query of a batch
struct Found {
  std::vector<int32_t> best_idx, best_dist, second_dist, best_level, second_level, second_idx;
  void reset(int nq) {
    for (auto* v : {&best_idx, &best_level, &second_level, &second_idx}) v->assign(nq, -1);
    best_dist.assign(nq, 256); second_dist.assign(nq, 256);
  }
  bool download(osh_orb_ctx* ctx) {
    return osh_orb_download(ctx, best_idx.data(), best_dist.data(), second_dist.data(), best_level.data(), second_level.data(), second_idx.data()) == OSH_OK;
  }
  Best2 at(int q) const {
    Best2 b;
    b.idx = best_idx[q]; b.dist = best_dist[q]; b.dist2 = second_dist[q]; b.level = best_level[q]; b.level2 = second_level[q];
    return b;
  }
};

// When the device result of a query no longer stands.  Occupancy only ever removes candidates, so the result can change only if
// a slot it names has been taken since: the best one where only the best is used, either where a ratio test follows.
enum Trigger { kBestTaken, kBestOrSecondTaken };
template <class Taken>
bool contested(const Found& f, int q, Trigger trigger, Taken taken) {
  if (f.best_idx[q] >= 0 && taken(f.best_idx[q])) return true;
  return trigger == kBestOrSecondTaken && f.second_idx[q] >= 0 && taken(f.second_idx[q]);
}

inline bool device_failed(const char* what) {
  std::fprintf(stderr, "ORBmatcher: device %s failed: %s\n", what, osh_last_error());
  return false;
}

// ---- searches over the target's grid: the device generates the candidates of every query's window itself
struct Search {
  std::vector<uint8_t> qdesc;            // [nq*32]
  std::vector<float> win;                // [nq*3] x, y, r of the query's GetFeaturesInArea call
  std::vector<int32_t> lev;              // [nq*2] minLevel, maxLevel
  std::vector<float> ur;                 // [nq*2] predicted u_right and tolerance (empty: no u_right test in this entry point)
  Found found;
  int nq() const { return (int)(win.size() / 3); }
  void add(const cv::Mat& d, float x, float y, float r, int minLevel, int maxLevel) {
    push_desc(qdesc, d, 0);
    win.push_back(x); win.push_back(y); win.push_back(r);
    lev.push_back(minLevel); lev.push_back(maxLevel);
  }
};

// the keypoint set that is searched
struct Train {
  const cv::Mat* desc = nullptr;
  int row0 = 0;                          // first descriptor row (and slot) of this keypoint set (right-camera keypoints: Nleft)
  std::vector<int32_t> level;
  std::vector<float> xy, uright;         // uright empty: no stereo test
  std::vector<uint8_t> skip;             // slots that are no candidates when the call starts
  float min_x = 0, min_y = 0, winv = 0, hinv = 0;
  int cols = 0, rows = 0;
  int n() const { return (int)level.size(); }
};

inline Train train_of_keys(const cv::Mat& desc, int row0, const std::vector<cv::KeyPoint>& keys, int n, float min_x, float min_y, float winv,
                           float hinv, int cols, int rows) {
  Train t;
  t.desc = &desc; t.row0 = row0;
  t.level.resize(n); t.xy.resize((size_t)n * 2); t.skip.assign(n, 0);
  for (int i = 0; i < n; ++i) { t.level[i] = keys[i].octave; t.xy[2 * i] = keys[i].pt.x; t.xy[2 * i + 1] = keys[i].pt.y; }
  t.min_x = min_x; t.min_y = min_y; t.winv = winv; t.hinv = hinv; t.cols = cols; t.rows = rows;
  return t;
}
// a frame without a second camera: mvKeysUn / mGrid
inline Train train_of(const Frame& F) {
  return train_of_keys(F.mDescriptors, 0, F.mvKeysUn, F.N, F.mnMinX, F.mnMinY, F.mfGridElementWidthInv, F.mfGridElementHeightInv, FRAME_GRID_COLS, FRAME_GRID_ROWS);
}
// one camera of a fisheye stereo frame: left keypoints mvKeys / mGrid / descriptor rows [0, Nleft), right keypoints mvKeysRight /
// mGridRight / rows [Nleft, N) (src/Frame.cc:406-416, 697-699)
inline Train train_of(const Frame& F, bool right) {
  return train_of_keys(F.mDescriptors, right ? F.Nleft : 0, right ? F.mvKeysRight : F.mvKeys, right ? F.N - F.Nleft : F.Nleft, F.mnMinX, F.mnMinY,
                       F.mfGridElementWidthInv, F.mfGridElementHeightInv, FRAME_GRID_COLS, FRAME_GRID_ROWS);
}
// the first N keypoints of a keyframe (mvKeysUn, mGrid: what KeyFrame::GetFeaturesInArea(x, y, r) walks)
inline Train train_of(const KeyFrame* pKF, int N) {
  return train_of_keys(pKF->mDescriptors, 0, pKF->mvKeysUn, N, (float)pKF->mnMinX, (float)pKF->mnMinY, pKF->mfGridElementWidthInv,
                       pKF->mfGridElementHeightInv, pKF->mnGridCols, pKF->mnGridRows);
}
// slots that are no candidates from the start: occupied(slot), slot = the index in the frame's / keyframe's own arrays
template <class Occupied>
void mark_occupied(Train& t, Occupied occupied) {
  for (int i = 0; i < t.n(); ++i) t.skip[i] = occupied(t.row0 + i) ? 1 : 0;
}
inline bool holds_observed_point(const std::vector<MapPoint*>& slots, int slot) { return slots[slot] && slots[slot]->Observations() > 0; }

// queries and the train side's grid become device resident; nullptr (and a message) on failure or for an empty search
inline osh_orb_ctx* upload_search(const Search& s, const Train& t) {
  if (s.nq() == 0) return nullptr;
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) return nullptr;
  osh_orb_batch b;
  b.n_pairs = 1; b.n_query = s.nq(); b.n_train = t.n();
  b.query_desc = s.qdesc.data(); b.train_desc = t.desc->ptr<uint8_t>(t.row0); b.train_level = t.level.data();
  b.cand_off = nullptr; b.cand_idx = nullptr; b.pair_cand_base = nullptr;
  osh_orb_grid g;
  g.train_xy = t.xy.data(); g.train_uright = t.uright.empty() ? nullptr : t.uright.data(); g.train_skip = t.skip.data();
  g.min_x = t.min_x; g.min_y = t.min_y; g.cell_w_inv = t.winv; g.cell_h_inv = t.hinv; g.cols = t.cols; g.rows = t.rows;
  g.query_window = s.win.data(); g.query_levels = s.lev.data(); g.query_uright = s.ur.empty() ? nullptr : s.ur.data();
  if (osh_orb_upload_grid(ctx, &b, &g) != OSH_OK) { device_failed("upload"); return nullptr; }
  return ctx;
}

// one batched device search of all queries; the candidates come from the train side's grid
inline bool device_search(Search& s, const Train& t) {
  s.found.reset(s.nq());
  if (s.nq() == 0) return true;
  osh_orb_ctx* ctx = upload_search(s, t);
  if (!ctx) return false;
  return (osh_orb_match(ctx) == OSH_OK && s.found.download(ctx)) || device_failed("search");
}

// the reference's scan of one query's candidates with the current occupancy (only for contested queries): `area` is the
// entry point's own GetFeaturesInArea call, the static filters are the ones the device applied
template <class Area>
Best2 rescan(const Search& s, int q, const Train& t, const std::vector<uint8_t>& occupied, Area area) {
  Best2 b;
  const uint32_t* qd = reinterpret_cast<const uint32_t*>(&s.qdesc[(size_t)q * 32]);
  const float r = s.win[3 * q + 2];
  if (!(r > 0.f)) return b;
  const int minLevel = s.lev[2 * q], maxLevel = s.lev[2 * q + 1];
  const std::vector<size_t> cand = area(s.win[3 * q], s.win[3 * q + 1], r, minLevel, maxLevel);
  for (const size_t i : cand) {
    const int idx = (int)i;
    if (t.skip[idx] || occupied[idx]) continue;
    if (t.level[idx] < minLevel || (maxLevel >= 0 && t.level[idx] > maxLevel)) continue;
    if (!s.ur.empty() && !t.uright.empty() && t.uright[idx] > 0) {
      const float er = std::fabs(s.ur[2 * q] - t.uright[idx]);
      if (er > s.ur[2 * q + 1]) continue;
    }
    b.offer(idx, hamming256(qd, t.desc->ptr<uint32_t>(t.row0 + idx)), t.level[idx]);
  }
  return b;
}

// the result of query q as the reference's sequential loop would have it: the device's, unless a slot it names has been taken
template <class Area>
Best2 best_of(const Search& s, int q, const Train& t, const std::vector<uint8_t>& taken, Trigger trigger, Area area) {
  if (contested(s.found, q, trigger, [&taken](int i) { return taken[i] != 0; })) return rescan(s, q, t, taken, area);
  return s.found.at(q);
}

// ---- searches over explicit candidate lists (cand_off / cand_idx): query q's candidates are idx[off[q] .. off[q + 1]), in order
inline osh_orb_ctx* upload_lists(const std::vector<uint8_t>& qdesc, const cv::Mat& train, int n_train, const std::vector<int32_t>& off,
                                 const std::vector<int32_t>& idx, const char* what) {
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) return nullptr;
  static const int64_t base = 0;
  static const int32_t none = 0;
  osh_orb_batch b;
  b.n_pairs = 1; b.n_query = (int)off.size() - 1; b.n_train = n_train;
  b.query_desc = qdesc.data(); b.train_desc = train.ptr<uint8_t>(0); b.train_level = nullptr;
  b.cand_off = off.data(); b.cand_idx = idx.empty() ? &none : idx.data(); b.pair_cand_base = &base;
  if (osh_orb_upload(ctx, &b) != OSH_OK) { device_failed(what); return nullptr; }
  return ctx;
}

// best / second-best distance of every query among its list, positions in list order
inline bool device_search_lists(const std::vector<uint8_t>& qdesc, const cv::Mat& train, int n_train, const std::vector<int32_t>& off,
                                const std::vector<int32_t>& idx, Found& found) {
  const int nq = (int)off.size() - 1;
  found.reset(nq);
  if (nq <= 0) return true;
  osh_orb_ctx* ctx = upload_lists(qdesc, train, n_train, off, idx, "search");
  if (!ctx) return false;
  return (osh_orb_match(ctx) == OSH_OK && found.download(ctx)) || device_failed("search");
}

// the Hamming distance of every (query, candidate) entry, in list order
inline bool device_list_distances(const std::vector<uint8_t>& qdesc, const cv::Mat& train, int n_train, const std::vector<int32_t>& off,
                                  const std::vector<int32_t>& idx, std::vector<int32_t>& dist) {
  dist.assign(idx.size(), 256);
  if ((int)off.size() - 1 <= 0 || idx.empty()) return true;
  osh_orb_ctx* ctx = upload_lists(qdesc, train, n_train, off, idx, "distances");
  if (!ctx) return false;
  return osh_orb_list_distances(ctx, dist.data()) == OSH_OK || device_failed("distances");
}

// the reference's candidate loop over query q's list, leaving out what is taken by now (only for contested queries)
template <class Taken>
Best2 rescan_list(const uint8_t* qdesc, const cv::Mat& train, const std::vector<int32_t>& off, const std::vector<int32_t>& idx, int q, Taken taken) {
  Best2 b;
  const uint32_t* qd = reinterpret_cast<const uint32_t*>(qdesc);
  for (int c = off[q]; c < off[q + 1]; ++c)
    if (!taken(idx[c])) b.offer(idx[c], hamming256(qd, train.ptr<uint32_t>(idx[c])), 0);
  return b;
}
template <class Taken>
Best2 best_of_list(const Found& found, const std::vector<uint8_t>& qdesc, const cv::Mat& train, const std::vector<int32_t>& off,
                   const std::vector<int32_t>& idx, int q, Trigger trigger, Taken taken) {
  if (contested(found, q, trigger, taken)) return rescan_list(&qdesc[(size_t)q * 32], train, off, idx, q, taken);
  return found.at(q);
}

// ---- rotation consistency (src/ORBmatcher.cc:2012-2053 and the histogram block of every entry point)
inline void three_maxima(const std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int n = (int)histo[i].size();
    if (n > max1) { max3 = max2; max2 = max1; max1 = n; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (n > max2) { max3 = max2; max2 = n; ind3 = ind2; ind2 = i; }
    else if (n > max3) { max3 = n; ind3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

struct RotHist {
  enum { kBins = 30 };                   // ORBmatcher::HISTO_LENGTH
  std::vector<int> bin[kBins];
  RotHist() { for (auto& b : bin) b.reserve(500); }
  // a match between keypoints of these two angles; the payload is what prune() hands back
  void add(float angle_a, float angle_b, int payload) {
    const float factor = 1.0f / kBins;
    float rot = angle_a - angle_b;
    if (rot < 0.0) rot += 360.0f;
    int b = (int)std::round(rot * factor);   // factor = 1/30 (sic): only bins 0..12 are ever hit
    if (b == kBins) b = 0;
    bin[b].push_back(payload);
  }
  // drop(payload) for every match outside the three dominant bins, in bin order
  template <class Drop>
  void prune(Drop drop) const {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    three_maxima(bin, kBins, ind1, ind2, ind3);
    for (int i = 0; i < kBins; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (const int payload : bin[i]) drop(payload);
    }
  }
};

// ---- visit(features of a, features of b) for every vocabulary node both feature vectors hold, in node order
template <class Visit>
void for_each_common_node(const DBoW2::FeatureVector& a, const DBoW2::FeatureVector& b, Visit visit) {
  DBoW2::FeatureVector::const_iterator ait = a.begin(), aend = a.end(), bit = b.begin(), bend = b.end();
  while (ait != aend && bit != bend) {
    if (ait->first == bit->first) { visit(ait->second, bit->second); ait++; bit++; }
    else if (ait->first < bit->first) ait = a.lower_bound(bit->first);
    else bit = b.lower_bound(ait->first);
  }
}

// ---- the scale gates of a map point projected into `target` (a Frame or a KeyFrame).  (px, py, pz) is the vector the entry
// point measures the distance on: from the camera centre to the point in the world frame, or the point in the camera frame.
// Inside the scale-invariance range; with view_gate, viewing angle below 60 degrees; then the predicted level and the window.
template <class Target>
bool scale_gate(MapPoint* pMP, const float px, const float py, const float pz, const bool view_gate, Target* target, const float th,
                int& nPredictedLevel, float& radius) {
  const float maxDistance = pMP->GetMaxDistanceInvariance();
  const float minDistance = pMP->GetMinDistanceInvariance();
  const float dist = std::sqrt(px * px + py * py + pz * pz);
  if (dist < minDistance || dist > maxDistance) return false;
  if (view_gate) {
    const Eigen::Vector3f Pn = pMP->GetNormal();
    if (px * Pn(0) + py * Pn(1) + pz * Pn(2) < 0.5 * dist) return false;
  }
  nPredictedLevel = pMP->PredictScale(dist, target);
  radius = th * target->mvScaleFactors[nPredictedLevel];
  return true;
}

}  // namespace ORB_SLAM3
