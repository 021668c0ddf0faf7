// ORBmatcher.cc -- ORB_SLAM3::ORBmatcher on MI355X (host side).
//
// Every entry point follows one scheme: build the queries, run ONE batched nearest / second-nearest Hamming search per
// keypoint set on the device (osh_orb_*), then replay the order-dependent part on the host in the reference's order.  For the
// projection searches (src/ORBmatcher.cc:84-120, 1743-1768, 1949-1964, 499-520) the candidates are generated on the device too:
// the host hands over the keypoint positions and every query's window (centre, radius, level range, u_right test) and
// osh_orb_upload_grid reproduces Frame::GetFeaturesInArea / KeyFrame::GetFeaturesInArea including their candidate order; the
// vocabulary and fuse searches hand over explicit candidate lists.  The sequential "this slot was just taken" rule is replayed
// exactly as SURVEY.md 8a prescribes: occupancy only ever removes candidates, so only a query whose result names a slot that was
// claimed earlier in the same call is scanned again with the reference's left-to-right loop.
//
// The scheme itself -- queries, search targets, device calls, the two rescans, the rotation histogram, the feature-vector walk,
// the scale gates -- lives once in orb_search.h.  What differs between the entry points is written at their call sites:
//
//   entry point                         rescan trigger          a slot is claimed by                     `continue`s worth knowing
//   SearchByProjection(F, points)       on the device (Nleft == -1)
//     ... fisheye stereo frame          best or second taken    points with Observations() > 0; a match   failed LEFT ratio test skips
//                                                               also claims its stereo partner (the       the point's right pass
//                                                               right pass: partner first, then itself)
//   SearchByProjection(F, LastFrame)    best taken              points with Observations() > 0            fisheye stereo: an EMPTY left
//                                                                                                         list skips the right search
//   SearchByProjection(F, pKF, found)   best taken              any match (and any point held at entry)
//   SearchByProjection(pKF, Scw, ...)   best taken              any match (and any point held at entry)
//   SearchBySim3, Fuse                  none: queries are independent / the replay works on the map itself
//   SearchByBoW (both)                  best or second taken    any match
//   SearchForInitialization             none: every candidate distance comes from the device, the loop itself is replayed
#include "ORBmatcher.h"

#include <climits>
#include <cstdlib>
#include <set>

#include "fuse_batch.h"
#include "orb_search.h"

namespace ORB_SLAM3 {

const int ORBmatcher::TH_HIGH = 100;
const int ORBmatcher::TH_LOW = 50;
const int ORBmatcher::HISTO_LENGTH = 30;
static_assert(ORBmatcher::HISTO_LENGTH == RotHist::kBins, "RotHist carries HISTO_LENGTH bins");

ORBmatcher::ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

int ORBmatcher::DescriptorDistance(const cv::Mat& a, const cv::Mat& b) { return hamming256(a.ptr<uint32_t>(), b.ptr<uint32_t>()); }

float ORBmatcher::RadiusByViewingCos(const float& viewCos) { return viewCos > 0.998 ? 2.5 : 4.0; }  // :215-221

void ORBmatcher::ComputeThreeMaxima(std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) { three_maxima(histo, L, ind1, ind2, ind3); }

namespace {

struct ThreadCtx {   // destroyed at thread exit (Tracking / LoopClosing threads come and go with System instances)
  osh_orb_ctx* ctx = nullptr;
  ~ThreadCtx() { if (ctx) osh_orb_destroy(ctx); }
};

}  // namespace

// the device of every thread's matcher context (and of the vocabulary copy ORBVocabulary::transform makes for it)
int HostMatcherDevice() {
  const char* dev = std::getenv("ORBSLAM3_HIP_DEVICE");
  return dev ? std::atoi(dev) : 0;
}

osh_orb_ctx* HostMatcherContext() {
  static thread_local ThreadCtx holder;
  if (!holder.ctx) {
    if (osh_orb_create(HostMatcherDevice(), &holder.ctx) != OSH_OK) {
      std::fprintf(stderr, "ORBmatcher: cannot create the HIP matcher context: %s\n", osh_last_error());
      holder.ctx = nullptr;
    }
  }
  return holder.ctx;
}

namespace {

// One keypoint set of a frame (all of it, or one camera of a fisheye stereo frame) during a search-and-replay: the target, the
// queries against it, and the slots claimed so far in this call.
struct Side {
  Frame& F;
  const bool right;
  Train t;
  Search s;
  std::vector<uint8_t> taken;
  Side(Frame& F_, Train t_, bool right_) : F(F_), right(right_), t(std::move(t_)), taken(t.n(), 0) {}
  std::vector<size_t> area(float x, float y, float r, int lo, int hi) const { return F.GetFeaturesInArea(x, y, r, lo, hi, right); }
  bool search() { return device_search(s, t); }
  Best2 best(int q, Trigger trigger) const {
    return best_of(s, q, t, taken, trigger, [this](float x, float y, float r, int lo, int hi) { return area(x, y, r, lo, hi); });
  }
  int slot(int idx) const { return t.row0 + idx; }
  void claim(int idx, MapPoint* pMP, bool blocks) {
    F.mvpMapPoints[slot(idx)] = pMP;
    if (blocks) taken[idx] = 1;
  }
};

// src/ORBmatcher.cc:43-213 on a fisheye stereo frame (Nleft != -1): per map point the left-camera pass (:60-141) and then the
// right-camera pass (:144-210).  Both passes of ALL points are searched on the device first (two batched launches, one per
// camera); the sequential part is replayed on the host in the reference's order.
// (A free function: the class declaration stays the reference's own, include/ORBmatcher.h.)
int search_local_points_rig(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th, const bool bFarPoints,
                            const float thFarPoints, const float mfNNratio) {
  auto RadiusByViewingCos = [](float viewCos) { return (float)(viewCos > 0.998 ? 2.5 : 4.0); };   // src/ORBmatcher.cc:215-221
  const bool bFactor = th != 1.0;
  auto occupied = [&F](int slot) { return holds_observed_point(F.mvpMapPoints, slot); };
  Side left(F, train_of(F, false), false), right(F, train_of(F, true), true);
  mark_occupied(left.t, occupied);                                      // :88-90 at call entry
  mark_occupied(right.t, occupied);                                     // :164-166
  struct Q { MapPoint* mp; int ql, qr; };
  std::vector<Q> qs;
  for (size_t iMP = 0; iMP < vpMapPoints.size(); iMP++) {
    MapPoint* pMP = vpMapPoints[iMP];
    if (!pMP->mbTrackInView && !pMP->mbTrackInViewR) continue;
    if (bFarPoints && pMP->mTrackDepth > thFarPoints) continue;
    if (pMP->isBad()) continue;
    Q q{pMP, -1, -1};
    if (pMP->mbTrackInView) {
      const int nPredictedLevel = pMP->mnTrackScaleLevel;
      float r = RadiusByViewingCos(pMP->mTrackViewCos);
      if (bFactor) r *= th;
      q.ql = left.s.nq();
      left.s.add(pMP->GetDescriptor(), pMP->mTrackProjX, pMP->mTrackProjY, r * F.mvScaleFactors[nPredictedLevel], nPredictedLevel - 1, nPredictedLevel);
    }
    if (pMP->mbTrackInViewR && pMP->mnTrackScaleLevelR != -1) {
      const int nPredictedLevel = pMP->mnTrackScaleLevelR;
      const float r = RadiusByViewingCos(pMP->mTrackViewCosR);   // no th factor in the right-camera pass (:148)
      q.qr = right.s.nq();
      right.s.add(pMP->GetDescriptor(), pMP->mTrackProjXR, pMP->mTrackProjYR, r * F.mvScaleFactors[nPredictedLevel], nPredictedLevel - 1, nPredictedLevel);
    }
    qs.push_back(q);
  }
  if (!left.search() || !right.search()) return 0;

  int nmatches = 0;
  // one camera's pass of one point (:123-139 / :196-207): the match takes its own slot and the slot of its stereo partner in the
  // other camera.  false: the ratio test failed
  auto pass = [&](Side& own, Side& other, const std::vector<int>& partner, const bool partner_first, int q, MapPoint* pMP, bool blocks) {
    const Best2 b = own.best(q, kBestOrSecondTaken);
    if (b.dist > ORBmatcher::TH_HIGH) return true;
    if (b.level == b.level2 && b.dist > mfNNratio * b.dist2) return false;
    if (!partner_first) own.claim(b.idx, pMP, blocks);
    if (partner[b.idx] != -1) { other.claim(partner[b.idx], pMP, blocks); nmatches++; }
    if (partner_first) own.claim(b.idx, pMP, blocks);
    nmatches++;
    return true;
  };
  for (const Q& q : qs) {
    const bool blocks = q.mp->Observations() > 0;   // only a point with observations keeps later points off its slots
    if (q.ql >= 0 && !pass(left, right, F.mvLeftToRightMatch, false, q.ql, q.mp, blocks)) continue;   // also skips this point's right-camera pass (:125-126)
    if (q.qr >= 0) pass(right, left, F.mvRightToLeftMatch, true, q.qr, q.mp, blocks);
  }
  return nmatches;
}

}  // namespace

// src/ORBmatcher.cc:43-213: Nleft == -1 layouts (monocular, rectified stereo, RGB-D) here, fisheye stereo frames above.
int ORBmatcher::SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th, const bool bFarPoints,
                                   const float thFarPoints) {
  if (F.Nleft != -1) return search_local_points_rig(F, vpMapPoints, th, bFarPoints, thFarPoints, mfNNratio);
  const bool bFactor = th != 1.0;
  Train t = train_of(F);
  t.uright = F.mvuRight;                                            // stereo consistency window (:92-97)
  mark_occupied(t, [&F](int slot) { return holds_observed_point(F.mvpMapPoints, slot); });   // :88-90 at call entry
  Search s;
  std::vector<MapPoint*> qMP;
  for (size_t iMP = 0; iMP < vpMapPoints.size(); iMP++) {
    MapPoint* pMP = vpMapPoints[iMP];
    if (!pMP->mbTrackInView && !pMP->mbTrackInViewR) continue;
    if (bFarPoints && pMP->mTrackDepth > thFarPoints) continue;
    if (pMP->isBad()) continue;
    if (!pMP->mbTrackInView) continue;
    const int nPredictedLevel = pMP->mnTrackScaleLevel;
    float r = RadiusByViewingCos(pMP->mTrackViewCos);   // window size depends on the viewing direction (:66-72)
    if (bFactor) r *= th;
    const float win = r * F.mvScaleFactors[nPredictedLevel];
    // candidates: GetFeaturesInArea(mTrackProjX, mTrackProjY, win, level-1, level) minus occupied slots, |ur - uR| <= win
    s.add(pMP->GetDescriptor(), pMP->mTrackProjX, pMP->mTrackProjY, win, nPredictedLevel - 1, nPredictedLevel);
    s.ur.push_back(pMP->mTrackProjXR); s.ur.push_back(win);
    qMP.push_back(pMP);
  }
  // search, acceptance rule (:123-139) and the sequential slot occupancy (:88-90) all on the device: osh_orb_match_local_points
  osh_orb_ctx* ctx = upload_search(s, t);
  if (!ctx) return 0;
  std::vector<uint8_t> blocks(qMP.size());
  for (size_t q = 0; q < qMP.size(); ++q) blocks[q] = qMP[q]->Observations() > 0 ? 1 : 0;
  std::vector<int32_t> assignment(F.N, -1);
  int32_t nmatches = 0;
  if (osh_orb_match_local_points(ctx, mfNNratio, TH_HIGH, nullptr, blocks.data(), assignment.data(), &nmatches, nullptr, nullptr) != OSH_OK)
    return device_failed("search");
  for (int i = 0; i < F.N; ++i) if (assignment[i] >= 0) F.mvpMapPoints[i] = qMP[assignment[i]];
  return nmatches;
}

// src/ORBmatcher.cc:1676-1887.  A frame without a second camera: one search among its keypoints with the u_right window
// (:1762-1767).  A fisheye stereo frame (Nleft != -1): per map point of the last frame the search among the current frame's LEFT
// keypoints (:1696-1792, no u_right test) and then, unless the left candidate list was empty (`continue` at :1732), among its RIGHT
// keypoints with the point moved through Trl and projected with mpCamera (:1794-1858).  All searches run on the device first.
int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono) {
  const Sophus::SE3f Tcw = CurrentFrame.GetPose();
  // twc = -Rcw^T tcw ; tlc = Tlw * twc  (forward / backward motion test, :1686-1693)
  const Eigen::Quaternionf qc = Tcw.unit_quaternion();
  const Sophus::SE3f Twc_rot(Eigen::Quaternionf(qc.w(), -qc.x(), -qc.y(), -qc.z()), Eigen::Vector3f(0, 0, 0));
  const Eigen::Vector3f mt(-Tcw.translation()(0), -Tcw.translation()(1), -Tcw.translation()(2));
  const Eigen::Vector3f twc = Twc_rot * mt;
  const Eigen::Vector3f tlc = LastFrame.GetPose() * twc;
  const bool bForward = tlc(2) > CurrentFrame.mb && !bMono;
  const bool bBackward = -tlc(2) > CurrentFrame.mb && !bMono;
  const bool rig = CurrentFrame.Nleft != -1;

  auto occupied = [&CurrentFrame](int slot) { return holds_observed_point(CurrentFrame.mvpMapPoints, slot); };
  Side left(CurrentFrame, rig ? train_of(CurrentFrame, false) : train_of(CurrentFrame), false);
  Side right(CurrentFrame, rig ? train_of(CurrentFrame, true) : Train(), true);   // no keypoints, no queries without a second camera
  if (!rig) left.t.uright = CurrentFrame.mvuRight;
  mark_occupied(left.t, occupied);
  mark_occupied(right.t, occupied);
  std::vector<int> qLast;  // index in LastFrame of every query
  for (int i = 0; i < LastFrame.N; i++) {
    MapPoint* pMP = LastFrame.mvpMapPoints[i];
    if (!pMP || LastFrame.mvbOutlier[i]) continue;
    const Eigen::Vector3f x3Dc = Tcw * pMP->GetWorldPos();
    const float invzc = 1.0 / x3Dc(2);
    if (invzc < 0) continue;
    const Eigen::Vector2f uv = CurrentFrame.mpCamera->project(x3Dc);
    if (uv(0) < CurrentFrame.mnMinX || uv(0) > CurrentFrame.mnMaxX) continue;
    if (uv(1) < CurrentFrame.mnMinY || uv(1) > CurrentFrame.mnMaxY) continue;
    // the octave is read from mvKeys also where there is no second camera (:1720-1721), unlike keypoint_of()
    const int nLastOctave = (LastFrame.Nleft == -1 || i < LastFrame.Nleft) ? LastFrame.mvKeys[i].octave : LastFrame.mvKeysRight[i - LastFrame.Nleft].octave;
    const float radius = th * CurrentFrame.mvScaleFactors[nLastOctave];   // window scales with the octave
    // level range by the motion direction (:1744-1750): forward -> [octave, inf), backward -> [0, octave], else octave +- 1
    int lo, hi;
    if (bForward) { lo = nLastOctave; hi = -1; }
    else if (bBackward) { lo = 0; hi = nLastOctave; }
    else { lo = nLastOctave - 1; hi = nLastOctave + 1; }
    left.s.add(pMP->GetDescriptor(), uv(0), uv(1), radius, lo, hi);
    if (rig) {
      const Eigen::Vector3f x3Dr = CurrentFrame.GetRelativePoseTrl() * x3Dc;       // :1795
      const Eigen::Vector2f uvr = CurrentFrame.mpCamera->project(x3Dr);            // :1796 (mpCamera, as in the reference)
      right.s.add(pMP->GetDescriptor(), uvr(0), uvr(1), radius, lo, hi);
    } else {
      left.s.ur.push_back(uv(0) - CurrentFrame.mbf * invzc); left.s.ur.push_back(radius);   // |ur - mvuRight| <= radius (:1762-1767)
    }
    qLast.push_back(i);
  }
  if (!left.search() || !right.search()) return 0;

  int nmatches = 0;
  RotHist hist;
  // the best candidate of query q on one side, accepted up to TH_HIGH; returns its index (-1: the query had no free candidate)
  auto replay = [&](Side& side, int q, MapPoint* pMP, float last_angle) {
    const Best2 b = side.best(q, kBestTaken);
    if (b.dist > TH_HIGH) return b.idx;
    side.claim(b.idx, pMP, pMP->Observations() > 0);
    nmatches++;
    if (mbCheckOrientation) hist.add(last_angle, keypoint_of(CurrentFrame, side.slot(b.idx)).angle, side.slot(b.idx));
    return b.idx;
  };
  for (int q = 0; q < left.s.nq(); ++q) {
    MapPoint* pMP = LastFrame.mvpMapPoints[qLast[q]];
    if (!rig) { replay(left, q, pMP, LastFrame.mvKeysUn[qLast[q]].angle); continue; }   // a last frame of the same layout: mvKeysUn
    const float last_angle = keypoint_of(LastFrame, qLast[q]).angle;                     // :1777-1779, 1842-1844
    // `if(vIndices2.empty()) continue;` (:1731-1732) also skips the right-camera search of this point: the device reports
    // "no candidate" for an empty list AND for a list whose entries are all occupied, so the (rare) no-candidate case asks
    if (replay(left, q, pMP, last_angle) < 0 &&
        left.area(left.s.win[3 * q], left.s.win[3 * q + 1], left.s.win[3 * q + 2], left.s.lev[2 * q], left.s.lev[2 * q + 1]).empty()) continue;
    replay(right, q, pMP, last_angle);
  }
  if (mbCheckOrientation) hist.prune([&](int slot) { CurrentFrame.mvpMapPoints[slot] = nullptr; nmatches--; });
  return nmatches;
}

// src/ORBmatcher.cc:1889-2010 (Tracking::Relocalization): the keyframe's map points are projected with the current
// pose estimate; best candidate only; a slot holding ANY map point is skipped (:1952) -- also one filled earlier in this
// call; accept bestDist <= ORBdist; rotation histogram with the keyframe keypoint's angle.
int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, const float th,
                                   const int ORBdist) {
  const Sophus::SE3f Tcw = CurrentFrame.GetPose();
  const Eigen::Vector3f Ow = Tcw.inverse().translation();
  const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();

  // on a fisheye stereo frame the reference searches the LEFT keypoints only here (GetFeaturesInArea's bRight defaults to false)
  Side cam(CurrentFrame, CurrentFrame.Nleft == -1 ? train_of(CurrentFrame) : train_of(CurrentFrame, false), false);
  mark_occupied(cam.t, [&CurrentFrame](int slot) { return CurrentFrame.mvpMapPoints[slot] != nullptr; });   // any matched slot (:1952)
  std::vector<int> qKF;  // keypoint index in pKF of every query
  for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
    MapPoint* pMP = vpMPs[i];
    if (!pMP || pMP->isBad() || sAlreadyFound.count(pMP)) continue;
    const Eigen::Vector3f x3Dw = pMP->GetWorldPos();
    const Eigen::Vector3f x3Dc = Tcw * x3Dw;
    const Eigen::Vector2f uv = CurrentFrame.mpCamera->project(x3Dc);
    if (uv(0) < CurrentFrame.mnMinX || uv(0) > CurrentFrame.mnMaxX) continue;
    if (uv(1) < CurrentFrame.mnMinY || uv(1) > CurrentFrame.mnMaxY) continue;
    // predicted scale level from the distance to the camera centre (:1922-1933); no depth and no viewing-angle gate here
    int nPredictedLevel;
    float radius;
    if (!scale_gate(pMP, x3Dw(0) - Ow(0), x3Dw(1) - Ow(1), x3Dw(2) - Ow(2), false, &CurrentFrame, th, nPredictedLevel, radius)) continue;
    cam.s.add(pMP->GetDescriptor(), uv(0), uv(1), radius, nPredictedLevel - 1, nPredictedLevel + 1);
    qKF.push_back((int)i);
  }
  if (!cam.search()) return 0;

  int nmatches = 0;
  RotHist hist;
  for (int q = 0; q < cam.s.nq(); ++q) {
    const Best2 b = cam.best(q, kBestTaken);
    if (b.dist > ORBdist) continue;
    cam.claim(b.idx, vpMPs[qKF[q]], true);   // any match blocks its slot
    nmatches++;
    if (mbCheckOrientation) {
      // chosen by the frame's layout alone (the candidates are left keypoints), the keyframe side is always mvKeysUn: not keypoint_of()
      const cv::KeyPoint& kpCF = CurrentFrame.Nleft == -1 ? CurrentFrame.mvKeysUn[b.idx] : CurrentFrame.mvKeys[b.idx];
      hist.add(pKF->mvKeysUn[qKF[q]].angle, kpCF.angle, b.idx);
    }
  }
  if (mbCheckOrientation) hist.prune([&](int slot) { CurrentFrame.mvpMapPoints[slot] = nullptr; nmatches--; });
  return nmatches;
}

namespace {

// Common body of the two Sim3 overloads (src/ORBmatcher.cc:427-532, 534-646).  They differ in how the point is projected
// (camera model object vs. the keyframe's pinhole intrinsics with a float 1/z) and in the extra vpMatchedKF output.
int search_by_sim3(KeyFrame* pKF, Sophus::Sim3f& Scw, const std::vector<MapPoint*>& vpPoints, const std::vector<KeyFrame*>* vpPointsKFs,
                   std::vector<MapPoint*>& vpMatched, std::vector<KeyFrame*>* vpMatchedKF, int th, float ratioHamming, int th_low) {
  const float &fx = pKF->fx, &fy = pKF->fy, &cx = pKF->cx, &cy = pKF->cy;
  const Eigen::Vector3f ts = Scw.translation();
  const float sc = Scw.scale();
  const Sophus::SE3f Tcw(Scw.rotationMatrix(), Eigen::Vector3f(ts(0) / sc, ts(1) / sc, ts(2) / sc));
  const Eigen::Vector3f Ow = Tcw.inverse().translation();
  std::set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
  spAlreadyFound.erase(static_cast<MapPoint*>(NULL));

  const int N = (int)vpMatched.size();
  Train t = train_of(pKF, N);
  mark_occupied(t, [&vpMatched](int slot) { return vpMatched[slot] != nullptr; });   // matched slots are skipped (:501-502)
  auto area = [pKF](float x, float y, float r, int, int) { return pKF->GetFeaturesInArea(x, y, r); };
  Search s;
  std::vector<int> qMP;
  for (int iMP = 0, iendMP = (int)vpPoints.size(); iMP < iendMP; iMP++) {
    MapPoint* pMP = vpPoints[iMP];
    if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
    const Eigen::Vector3f p3Dw = pMP->GetWorldPos();
    const Eigen::Vector3f p3Dc = Tcw * p3Dw;
    if (p3Dc(2) < 0.0) continue;
    float u, v;
    if (!vpPointsKFs) {
      const Eigen::Vector2f uv = pKF->mpCamera->project(p3Dc);   // :467
      u = uv(0); v = uv(1);
    } else {
      const float invz = 1 / p3Dc(2);                            // :573-578
      const float x = p3Dc(0) * invz, y = p3Dc(1) * invz;
      u = fx * x + cx; v = fy * y + cy;
    }
    if (!pKF->IsInImage(u, v)) continue;
    int nPredictedLevel;   // distance from the camera centre, viewing angle below 60 degrees (:474-489)
    float radius;
    if (!scale_gate(pMP, p3Dw(0) - Ow(0), p3Dw(1) - Ow(1), p3Dw(2) - Ow(2), true, pKF, th, nPredictedLevel, radius)) continue;
    // KeyFrame::GetFeaturesInArea(u, v, radius) has no level arguments; the loop keeps levels L-1 .. L (:504-507)
    s.add(pMP->GetDescriptor(), u, v, radius, std::max(nPredictedLevel - 1, 0), nPredictedLevel);
    qMP.push_back(iMP);
  }
  if (!device_search(s, t)) return 0;

  int nmatches = 0;
  std::vector<uint8_t> taken(N, 0);
  for (int q = 0; q < s.nq(); ++q) {
    const Best2 b = best_of(s, q, t, taken, kBestTaken, area);
    if (b.idx >= 0 && b.dist <= th_low * ratioHamming) {          // int <= float (:523,636)
      vpMatched[b.idx] = vpPoints[qMP[q]];
      if (vpMatchedKF) (*vpMatchedKF)[b.idx] = (*vpPointsKFs)[qMP[q]];
      taken[b.idx] = 1;                                           // any match blocks its slot
      nmatches++;
    }
  }
  return nmatches;
}

}  // namespace

int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const std::vector<MapPoint*>& vpPoints,
                                   std::vector<MapPoint*>& vpMatched, int th, float ratioHamming) {
  return search_by_sim3(pKF, Scw, vpPoints, nullptr, vpMatched, nullptr, th, ratioHamming, TH_LOW);
}

int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3<float>& Scw, const std::vector<MapPoint*>& vpPoints,
                                   const std::vector<KeyFrame*>& vpPointsKFs, std::vector<MapPoint*>& vpMatched,
                                   std::vector<KeyFrame*>& vpMatchedKF, int th, float ratioHamming) {
  return search_by_sim3(pKF, Scw, vpPoints, &vpPointsKFs, vpMatched, &vpMatchedKF, th, ratioHamming, TH_LOW);
}

namespace {

// One direction of SearchBySim3 (src/ORBmatcher.cc:1497-1576 / :1578-1657): the map points of keyframe `from` that are not matched
// yet, moved into the camera of keyframe `to` by Tfw and then S, searched among `to`'s keypoints of levels L-1 .. L around the
// projection.  No slot occupancy: every query is independent, so the device result IS the loop's result.
bool sim3_direction(KeyFrame* to_kf, const float fx, const float fy, const float cx, const float cy, const Sophus::SE3f& Tfw, const Sophus::Sim3f& S,
                    const std::vector<MapPoint*>& vpFrom, const std::vector<bool>& vbAlready, int n_to, float th, int th_high, std::vector<int>& vnMatch) {
  Train t = train_of(to_kf, n_to);
  Search s;
  std::vector<int> qSlot;
  for (int i = 0, n = (int)vpFrom.size(); i < n; ++i) {
    MapPoint* pMP = vpFrom[i];
    if (!pMP || vbAlready[i]) continue;
    if (pMP->isBad()) continue;
    const Eigen::Vector3f p3Dw = pMP->GetWorldPos();
    const Eigen::Vector3f p3Df = Tfw * p3Dw;
    const Eigen::Vector3f p3Dt = S * p3Df;
    if (p3Dt(2) < 0.0) continue;                                   // depth must be positive
    const float invz = 1.0 / p3Dt(2);
    const float x = p3Dt(0) * invz, y = p3Dt(1) * invz;
    const float u = fx * x + cx, v = fy * y + cy;
    if (!to_kf->IsInImage(u, v)) continue;
    int nPredictedLevel;   // the distance is the norm of the point in the target camera frame (:1527, 1607); no viewing-angle gate
    float radius;
    if (!scale_gate(pMP, p3Dt(0), p3Dt(1), p3Dt(2), false, to_kf, th, nPredictedLevel, radius)) continue;
    s.add(pMP->GetDescriptor(), u, v, radius, std::max(nPredictedLevel - 1, 0), nPredictedLevel);
    qSlot.push_back(i);
  }
  if (!device_search(s, t)) return false;
  for (int q = 0; q < s.nq(); ++q)
    if (s.found.best_idx[q] >= 0 && s.found.best_dist[q] <= th_high) vnMatch[qSlot[q]] = s.found.best_idx[q];
  return true;
}

}  // namespace

// src/ORBmatcher.cc:1457-1674: both directions as one batched device search each, then the agreement check (:1659-1673).
int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const Sophus::Sim3f& S12, const float th) {
  const Sophus::SE3f T1w = pKF1->GetPose();
  const Sophus::SE3f T2w = pKF2->GetPose();
  const Sophus::Sim3f S21 = S12.inverse();
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  const int N1 = (int)vpMapPoints1.size();
  const std::vector<MapPoint*> vpMapPoints2 = pKF2->GetMapPointMatches();
  const int N2 = (int)vpMapPoints2.size();
  std::vector<bool> vbAlreadyMatched1(N1, false), vbAlreadyMatched2(N2, false);
  for (int i = 0; i < N1; i++) {
    MapPoint* pMP = vpMatches12[i];
    if (pMP) {
      vbAlreadyMatched1[i] = true;
      const int idx2 = std::get<0>(pMP->GetIndexInKeyFrame(pKF2));
      if (idx2 >= 0 && idx2 < N2) vbAlreadyMatched2[idx2] = true;
    }
  }
  std::vector<int> vnMatch1(N1, -1), vnMatch2(N2, -1);
  // the reference projects with pKF1's fx fy cx cy in BOTH directions (:1459-1462, 1520-1521, 1600-1601)
  const float fx = pKF1->fx, fy = pKF1->fy, cx = pKF1->cx, cy = pKF1->cy;
  if (!sim3_direction(pKF2, fx, fy, cx, cy, T1w, S21, vpMapPoints1, vbAlreadyMatched1, N2, th, TH_HIGH, vnMatch1)) return 0;
  if (!sim3_direction(pKF1, fx, fy, cx, cy, T2w, S12, vpMapPoints2, vbAlreadyMatched2, N1, th, TH_HIGH, vnMatch2)) return 0;
  int nFound = 0;
  for (int i1 = 0; i1 < N1; i1++) {
    const int idx2 = vnMatch1[i1];
    if (idx2 >= 0 && vnMatch2[idx2] == i1) { vpMatches12[i1] = vpMapPoints2[idx2]; nFound++; }
  }
  return nFound;
}

// src/ORBmatcher.cc:648-763 (monocular map initialisation).  The candidates of every level-0 keypoint of F1 are the level-0 features
// of F2 in the window around its previous match; the device returns the distance of every (keypoint, candidate) entry in one launch.
// The loop itself is order dependent -- a candidate is skipped while the distance it was last matched with is not larger
// (vMatchedDistance), and a new match displaces the old one of the same feature -- and is replayed as written.
int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, std::vector<cv::Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize) {
  int nmatches = 0;
  vnMatches12 = std::vector<int>(F1.mvKeysUn.size(), -1);
  RotHist hist;
  std::vector<int> vMatchedDistance(F2.mvKeysUn.size(), INT_MAX);
  std::vector<int> vnMatches21(F2.mvKeysUn.size(), -1);
  // queries: the level-0 keypoints with a non-empty window, in order
  std::vector<int> q1;
  std::vector<uint8_t> qdesc;
  std::vector<int32_t> off(1, 0), idx;
  for (size_t i1 = 0, iend1 = F1.mvKeysUn.size(); i1 < iend1; i1++) {
    const int level1 = F1.mvKeysUn[i1].octave;
    if (level1 > 0) continue;
    const std::vector<size_t> vIndices2 = F2.GetFeaturesInArea(vbPrevMatched[i1].x, vbPrevMatched[i1].y, (float)windowSize, level1, level1);
    if (vIndices2.empty()) continue;
    for (size_t i2 : vIndices2) idx.push_back((int32_t)i2);
    off.push_back((int32_t)idx.size());
    q1.push_back((int)i1);
    push_desc(qdesc, F1.mDescriptors, (int)i1);
  }
  std::vector<int32_t> dist;
  if (!device_list_distances(qdesc, F2.mDescriptors, F2.mDescriptors.rows, off, idx, dist)) return 0;
  for (size_t q = 0; q < q1.size(); ++q) {
    const int i1 = q1[q];
    int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
    for (int e = off[q]; e < off[q + 1]; ++e) {
      const int i2 = idx[e], d = dist[e];
      if (vMatchedDistance[i2] <= d) continue;
      if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestIdx2 = i2; }
      else if (d < bestDist2) bestDist2 = d;
    }
    if (bestDist <= TH_LOW) {
      if (bestDist < (float)bestDist2 * mfNNratio) {
        if (vnMatches21[bestIdx2] >= 0) { vnMatches12[vnMatches21[bestIdx2]] = -1; nmatches--; }
        vnMatches12[i1] = bestIdx2;
        vnMatches21[bestIdx2] = i1;
        vMatchedDistance[bestIdx2] = bestDist;
        nmatches++;
        if (mbCheckOrientation) hist.add(F1.mvKeysUn[i1].angle, F2.mvKeysUn[bestIdx2].angle, i1);
      }
    }
  }
  // a match that was displaced since it entered the histogram is not dropped twice
  if (mbCheckOrientation) hist.prune([&](int idx1) { if (vnMatches12[idx1] >= 0) { vnMatches12[idx1] = -1; nmatches--; } });
  for (size_t i1 = 0, iend1 = vnMatches12.size(); i1 < iend1; i1++)      // update prev matched
    if (vnMatches12[i1] >= 0) vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt;
  return nmatches;
}

// src/ORBmatcher.cc:907-1146.  No step of this search depends on an earlier one (vbMatched2 is read but never set), so every
// unmatched feature of keyframe 1 is a query whose candidates are the unmatched features of keyframe 2 in the same vocabulary
// node.  The device returns the distance of every (query, candidate) entry in one launch; the choice among the candidates --
// the reference's loop with its `dist > bestDist` rule (a later candidate at the same distance wins), the epipole test and the
// epipolar constraint, which is a virtual call on the camera object -- runs on the host over the entries within TH_LOW only.
int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                                       const bool bOnlyStereo, const bool bCoarse) {
  // Compute epipole in second image
  Sophus::SE3f T1w = pKF1->GetPose();
  Sophus::SE3f T2w = pKF2->GetPose();
  Sophus::SE3f Tw2 = pKF2->GetPoseInverse();
  Eigen::Vector3f Cw = pKF1->GetCameraCenter();
  Eigen::Vector3f C2 = T2w * Cw;
  Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
  Sophus::SE3f T12;
  Sophus::SE3f Tll, Tlr, Trl, Trr;
  Eigen::Matrix3f R12;
  Eigen::Vector3f t12;
  GeometricCamera *pCamera1 = pKF1->mpCamera, *pCamera2 = pKF2->mpCamera;
  if (!pKF1->mpCamera2 && !pKF2->mpCamera2) {
    T12 = T1w * Tw2;
    R12 = T12.rotationMatrix();
    t12 = T12.translation();
  } else {
    Sophus::SE3f Tr1w = pKF1->GetRightPose();
    Sophus::SE3f Twr2 = pKF2->GetRightPoseInverse();
    Tll = T1w * Tw2; Tlr = T1w * Twr2; Trl = Tr1w * Tw2; Trr = Tr1w * Twr2;
  }
  Eigen::Matrix3f Rll = Tll.rotationMatrix(), Rlr = Tlr.rotationMatrix(), Rrl = Trl.rotationMatrix(), Rrr = Trr.rotationMatrix();
  Eigen::Vector3f tll = Tll.translation(), tlr = Tlr.translation(), trl = Trl.translation(), trr = Trr.translation();

  // ---- queries and candidate lists in the order of the vocabulary walk
  std::vector<int> q1;
  std::vector<uint8_t> qdesc;
  std::vector<int32_t> off(1, 0), idx;
  for_each_common_node(pKF1->mFeatVec, pKF2->mFeatVec, [&](const std::vector<unsigned int>& feats1, const std::vector<unsigned int>& feats2) {
    for (const size_t idx1 : feats1) {
      if (pKF1->GetMapPoint(idx1)) continue;                       // already a MapPoint: skip
      const bool bStereo1 = (!pKF1->mpCamera2 && pKF1->mvuRight[idx1] >= 0);
      if (bOnlyStereo && !bStereo1) continue;
      for (const size_t idx2 : feats2) {
        if (pKF2->GetMapPoint(idx2)) continue;                     // already matched / already a MapPoint
        const bool bStereo2 = (!pKF2->mpCamera2 && pKF2->mvuRight[idx2] >= 0);
        if (bOnlyStereo && !bStereo2) continue;
        idx.push_back((int32_t)idx2);
      }
      off.push_back((int32_t)idx.size());
      q1.push_back((int)idx1);
      push_desc(qdesc, pKF1->mDescriptors, (int)idx1);
    }
  });
  std::vector<int32_t> dist;
  if (!device_list_distances(qdesc, pKF2->mDescriptors, pKF2->mDescriptors.rows, off, idx, dist)) return 0;

  int nmatches = 0;
  std::vector<int> vMatches12(pKF1->N, -1);
  RotHist hist;
  for (size_t q = 0; q < q1.size(); ++q) {
    const size_t idx1 = (size_t)q1[q];
    const bool bStereo1 = (!pKF1->mpCamera2 && pKF1->mvuRight[idx1] >= 0);
    const cv::KeyPoint& kp1 = keypoint_of(pKF1, (int)idx1);
    const bool bRight1 = (pKF1->NLeft == -1 || (int)idx1 < pKF1->NLeft) ? false : true;
    int bestDist = TH_LOW;
    int bestIdx2 = -1;
    for (int e = off[q]; e < off[q + 1]; ++e) {
      const size_t idx2 = (size_t)idx[e];
      const int d = dist[e];
      if (d > TH_LOW || d > bestDist) continue;
      const bool bStereo2 = (!pKF2->mpCamera2 && pKF2->mvuRight[idx2] >= 0);
      const cv::KeyPoint& kp2 = keypoint_of(pKF2, (int)idx2);
      const bool bRight2 = (pKF2->NLeft == -1 || (int)idx2 < pKF2->NLeft) ? false : true;
      if (!bStereo1 && !bStereo2 && !pKF1->mpCamera2) {
        const float distex = ep(0) - kp2.pt.x;
        const float distey = ep(1) - kp2.pt.y;
        if (distex * distex + distey * distey < 100 * pKF2->mvScaleFactors[kp2.octave]) continue;
      }
      if (pKF1->mpCamera2 && pKF2->mpCamera2) {
        if (bRight1 && bRight2) { R12 = Rrr; t12 = trr; T12 = Trr; pCamera1 = pKF1->mpCamera2; pCamera2 = pKF2->mpCamera2; }
        else if (bRight1 && !bRight2) { R12 = Rrl; t12 = trl; T12 = Trl; pCamera1 = pKF1->mpCamera2; pCamera2 = pKF2->mpCamera; }
        else if (!bRight1 && bRight2) { R12 = Rlr; t12 = tlr; T12 = Tlr; pCamera1 = pKF1->mpCamera; pCamera2 = pKF2->mpCamera2; }
        else { R12 = Rll; t12 = tll; T12 = Tll; pCamera1 = pKF1->mpCamera; pCamera2 = pKF2->mpCamera; }
      }
      if (bCoarse || pCamera1->epipolarConstrain(pCamera2, kp1, kp2, R12, t12, pKF1->mvLevelSigma2[kp1.octave], pKF2->mvLevelSigma2[kp2.octave])) {
        bestIdx2 = (int)idx2;
        bestDist = d;
      }
    }
    if (bestIdx2 >= 0) {
      vMatches12[idx1] = bestIdx2;
      nmatches++;
      if (mbCheckOrientation) hist.add(kp1.angle, keypoint_of(pKF2, bestIdx2).angle, (int)idx1);
    }
  }
  if (mbCheckOrientation) hist.prune([&](int idx1) { vMatches12[idx1] = -1; nmatches--; });
  vMatchedPairs.clear();
  vMatchedPairs.reserve(nmatches);
  for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
    if (vMatches12[i] < 0) continue;
    vMatchedPairs.push_back(std::make_pair(i, (size_t)vMatches12[i]));
  }
  return nmatches;
}

// The host part of fuse_search, with external linkage (declared in fuse_batch.h) so that the test library can read what one Fuse call
// decides per point before its device search: qOf[i] = query of point i or -1; query q's candidates are idx[off[q] .. off[q + 1]).
void FuseCandidateLists(KeyFrame* pKF, const Sophus::SE3f& Tcw, const Eigen::Vector3f& Ow, GeometricCamera* pCamera, const std::vector<MapPoint*>& vpMapPoints,
                        const float th, const bool bRight, const bool chi2_gate, std::vector<int>& qOf, std::vector<uint8_t>& qdesc,
                        std::vector<int32_t>& off, std::vector<int32_t>& idx) {
  const float& bf = pKF->mbf;
  const int nMPs = (int)vpMapPoints.size();
  qOf.assign(nMPs, -1);
  qdesc.clear(); idx.clear(); off.assign(1, 0);
  int nq = 0;
  for (int i = 0; i < nMPs; i++) {
    MapPoint* pMP = vpMapPoints[i];
    if (!pMP) continue;
    const Eigen::Vector3f p3Dw = pMP->GetWorldPos();
    const Eigen::Vector3f p3Dc = Tcw * p3Dw;
    if (p3Dc(2) < 0.0f) continue;                                   // depth must be positive
    const float invz = 1 / p3Dc(2);
    const Eigen::Vector2f uv = pCamera->project(p3Dc);
    if (!pKF->IsInImage(uv(0), uv(1))) continue;                    // point must be inside the image
    const float ur = uv(0) - bf * invz;
    int nPredictedLevel;   // inside the scale pyramid of the image, viewing angle below 60 degrees
    float radius;
    if (!scale_gate(pMP, p3Dw(0) - Ow(0), p3Dw(1) - Ow(1), p3Dw(2) - Ow(2), true, pKF, th, nPredictedLevel, radius)) continue;
    const std::vector<size_t> vIndices = pKF->GetFeaturesInArea(uv(0), uv(1), radius, bRight);
    if (vIndices.empty()) continue;
    for (size_t k : vIndices) {
      // k counts within the searched camera here, and the Sim3 overload reads mvKeysUn whatever the layout (:1420): not keypoint_of()
      const cv::KeyPoint& kp = (!chi2_gate || pKF->NLeft == -1) ? pKF->mvKeysUn[k] : (!bRight) ? pKF->mvKeys[k] : pKF->mvKeysRight[k];
      const int& kpLevel = kp.octave;
      if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
      if (chi2_gate) {
        const float ex = uv(0) - kp.pt.x, ey = uv(1) - kp.pt.y;
        if (pKF->mvuRight[k] >= 0) {                                // reprojection error in stereo
          const float er = ur - pKF->mvuRight[k];
          const float e2 = ex * ex + ey * ey + er * er;
          if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 7.8) continue;
        } else {
          const float e2 = ex * ex + ey * ey;
          if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 5.99) continue;
        }
      }
      idx.push_back((int32_t)(bRight ? k + pKF->NLeft : k));
    }
    off.push_back((int32_t)idx.size());
    push_desc(qdesc, pMP->GetDescriptor(), 0);
    qOf[i] = nq++;
  }
}

// src/ORBmatcher.cc:1148-1338.  Every map point is projected into the keyframe and its candidate list (the features in the search
// radius that pass the level and the reprojection-chi2 gates, in GetFeaturesInArea's order) is formed up front: none of that depends
// on what the loop does to earlier points.  ONE batched device search gives the best candidate of every point; the part that is
// order dependent -- "already in the keyframe", Replace in either direction, AddObservation / AddMapPoint -- is replayed in the
// reference's order on the map itself.
namespace {

// The part of both Fuse overloads that does not depend on what their loops do to the map: per map point the projection gates
// (src/ORBmatcher.cc:1196-1260 / 1372-1412) and the candidate list -- the features of GetFeaturesInArea, in its order, that pass the
// level gate and (first overload, chi2_gate) the reprojection-error gate -- then ONE batched device search over the lists.
// qOf[i] = query of point i or -1; best / bestD by query.
bool fuse_search(KeyFrame* pKF, const Sophus::SE3f& Tcw, const Eigen::Vector3f& Ow, GeometricCamera* pCamera, const std::vector<MapPoint*>& vpMapPoints,
                 const float th, const bool bRight, const bool chi2_gate, std::vector<int>& qOf, std::vector<int32_t>& best, std::vector<int32_t>& bestD) {
  std::vector<uint8_t> qdesc;
  std::vector<int32_t> off, idx;
  FuseCandidateLists(pKF, Tcw, Ow, pCamera, vpMapPoints, th, bRight, chi2_gate, qOf, qdesc, off, idx);
  Found found;
  best.clear(); bestD.clear();
  if (off.size() > 1 && !device_search_lists(qdesc, pKF->mDescriptors, pKF->mDescriptors.rows, off, idx, found)) return false;
  best.swap(found.best_idx); bestD.swap(found.best_dist);
  return true;
}

}  // namespace

int ORBmatcher::Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const float th, const bool bRight) {
  GeometricCamera* pCamera;
  Sophus::SE3f Tcw;
  Eigen::Vector3f Ow;
  if (bRight) { Tcw = pKF->GetRightPose(); Ow = pKF->GetRightCameraCenter(); pCamera = pKF->mpCamera2; }
  else { Tcw = pKF->GetPose(); Ow = pKF->GetCameraCenter(); pCamera = pKF->mpCamera; }
  const int nMPs = (int)vpMapPoints.size();
  std::vector<int> qOf;
  std::vector<int32_t> best, bestD;
  if (!fuse_search(pKF, Tcw, Ow, pCamera, vpMapPoints, th, bRight, true, qOf, best, bestD)) return 0;

  int nFused = 0;
  for (int i = 0; i < nMPs; i++) {
    MapPoint* pMP = vpMapPoints[i];
    if (!pMP) continue;
    if (pMP->isBad()) continue;
    else if (pMP->IsInKeyFrame(pKF)) continue;
    if (qOf[i] < 0) continue;
    const int bestDist = bestD[qOf[i]], bestIdx = best[qOf[i]];
    if (bestIdx >= 0 && bestDist <= TH_LOW) {                       // already a MapPoint there: replace, otherwise add the measurement
      MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) {
          if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
          else pMPinKF->Replace(pMP);
        }
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
  }
  return nFused;
}

// src/ORBmatcher.cc:1340-1455 (loop closing / map merging): the same search through a Sim3 pose, no reprojection-error gate; a point
// whose best feature already holds a map point is reported in vpReplacePoint instead of being replaced.
int ORBmatcher::Fuse(KeyFrame* pKF, Sophus::Sim3f& Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint) {
  const Eigen::Vector3f ts = Scw.translation();
  const float sc = Scw.scale();
  const Sophus::SE3f Tcw(Scw.rotationMatrix(), Eigen::Vector3f(ts(0) / sc, ts(1) / sc, ts(2) / sc));
  const Eigen::Vector3f Ow = Tcw.inverse().translation();
  const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();    // as found at entry: the loop does not update it
  const int nPoints = (int)vpPoints.size();
  std::vector<int> qOf;
  std::vector<int32_t> best, bestD;
  if (!fuse_search(pKF, Tcw, Ow, pKF->mpCamera, vpPoints, th, false, false, qOf, best, bestD)) return 0;
  int nFused = 0;
  for (int iMP = 0; iMP < nPoints; iMP++) {
    MapPoint* pMP = vpPoints[iMP];
    if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
    if (qOf[iMP] < 0) continue;
    const int bestDist = bestD[qOf[iMP]], bestIdx = best[qOf[iMP]];
    if (bestIdx >= 0 && bestDist <= TH_LOW) {
      MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
  }
  return nFused;
}

// ---- FuseBatch: pack, one search, replay (fuse_batch.h)
namespace {

// the Sim3 overload's pose and centre, as Fuse(KeyFrame*, Sim3f&, ...) forms them
void sim3_pose(const Sophus::Sim3f& Scw, Sophus::SE3f& Tcw, Eigen::Vector3f& Ow) {
  const Eigen::Vector3f ts = Scw.translation();
  const float sc = Scw.scale();
  Tcw = Sophus::SE3f(Scw.rotationMatrix(), Eigen::Vector3f(ts(0) / sc, ts(1) / sc, ts(2) / sc));
  Ow = Tcw.inverse().translation();
}

bool fuse_batch_search(FuseBatchPack& pk, int mode, bool on_host, FuseBatchFound& found) {
  pk.bind();
  found.size(pk.targets.size() * (size_t)pk.P);
  if (pk.targets.empty() || pk.P == 0) return true;
  if (on_host) return FuseSearchOnHost(pk, mode, found);
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) return false;
  return osh_orb_fuse_search(ctx, (int32_t)pk.targets.size(), pk.targets.data(), &pk.points, mode, &found.result) == OSH_OK || device_failed("fuse batch search");
}

}  // namespace

std::vector<int> ORBmatcher::FuseBatch(const std::vector<FuseTarget>& targets, const std::vector<MapPoint*>& vpMapPoints) {
  const int K = (int)targets.size(), nMPs = (int)vpMapPoints.size();
  std::vector<int> fused(K, 0);
  FuseBatchPack pk;
  pk.set_points(vpMapPoints);
  for (const FuseTarget& t : targets) {
    KeyFrame* pKF = t.pKF;
    if (t.bRight) pk.add_target(pKF, pKF->GetRightPose(), pKF->GetRightCameraCenter(), pKF->mpCamera2, t.th, true, true);
    else pk.add_target(pKF, pKF->GetPose(), pKF->GetCameraCenter(), pKF->mpCamera, t.th, false, true);
  }
  FuseBatchFound found;
  if (!fuse_batch_search(pk, OSH_FUSE_CHI2, mbFuseBatchSearchOnHost, found)) {
    for (int k = 0; k < K; ++k) fused[k] = Fuse(targets[k].pKF, vpMapPoints, targets[k].th, targets[k].bRight);
    return fused;
  }
  FuseBatchReplay replay(pk, found, OSH_FUSE_CHI2, TH_LOW);
  for (int k = 0; k < K; ++k) {
    KeyFrame* pKF = targets[k].pKF;
    int nFused = 0;
    for (int i = 0; i < nMPs; i++) {                                  // Fuse, csrc/host/ORBmatcher.cc: the same loop
      MapPoint* pMP = vpMapPoints[i];
      if (!pMP) continue;
      if (pMP->isBad()) continue;
      else if (pMP->IsInKeyFrame(pKF)) continue;
      int bestIdx, bestDist;
      if (!replay.best_of(k, i, pMP, bestIdx, bestDist)) continue;
      if (bestIdx >= 0 && bestDist <= TH_LOW) {
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
          if (!pMPinKF->isBad()) {
            if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
            else pMPinKF->Replace(pMP);
          }
        } else {
          pMP->AddObservation(pKF, bestIdx);
          pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
      }
    }
    fused[k] = nFused;
    if (k + 1 < K) replay.mark_stale(vpMapPoints);
  }
  mnFuseBatchResearched += replay.researched; mnFuseBatchResearchedChanged += replay.changed;
  return fused;
}

std::vector<int> ORBmatcher::FuseBatch(const std::vector<std::pair<KeyFrame*, Sophus::Sim3f>>& targets, const std::vector<MapPoint*>& vpPoints, float th,
                                       std::vector<std::vector<MapPoint*>>& vvpReplacePoints, AfterTarget after) {
  const int K = (int)targets.size(), nPoints = (int)vpPoints.size();
  std::vector<int> fused(K, 0);
  vvpReplacePoints.assign(K, std::vector<MapPoint*>(nPoints, static_cast<MapPoint*>(nullptr)));
  FuseBatchPack pk;
  pk.set_points(vpPoints);
  for (const auto& t : targets) {
    Sophus::SE3f Tcw;
    Eigen::Vector3f Ow;
    sim3_pose(t.second, Tcw, Ow);
    pk.add_target(t.first, Tcw, Ow, t.first->mpCamera, th, false, false);
  }
  FuseBatchFound found;
  if (!fuse_batch_search(pk, OSH_FUSE_SIM3, mbFuseBatchSearchOnHost, found)) {
    for (int k = 0; k < K; ++k) {
      Sophus::Sim3f Scw = targets[k].second;
      fused[k] = Fuse(targets[k].first, Scw, vpPoints, th, vvpReplacePoints[k]);
      if (after) after(k);
    }
    return fused;
  }
  FuseBatchReplay replay(pk, found, OSH_FUSE_SIM3, TH_LOW);
  for (int k = 0; k < K; ++k) {
    KeyFrame* pKF = targets[k].first;
    const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();    // as found when this target's turn comes, as at Fuse's entry
    std::vector<MapPoint*>& vpReplacePoint = vvpReplacePoints[k];
    int nFused = 0;
    for (int iMP = 0; iMP < nPoints; iMP++) {
      MapPoint* pMP = vpPoints[iMP];
      if (!pMP) continue;                                             // the reference dereferences a null entry here
      if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
      int bestIdx, bestDist;
      if (!replay.best_of(k, iMP, pMP, bestIdx, bestDist)) continue;
      if (bestIdx >= 0 && bestDist <= TH_LOW) {
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
          if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
        } else {
          pMP->AddObservation(pKF, bestIdx);
          pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
      }
    }
    fused[k] = nFused;
    if (after) after(k);
    if (k + 1 < K) replay.mark_stale(vpPoints);
  }
  mnFuseBatchResearched += replay.researched; mnFuseBatchResearchedChanged += replay.changed;
  return fused;
}

// src/ORBmatcher.cc:223-420.  The candidate loops of every keyframe feature run as batched device searches over the feature
// lists of its vocabulary node (one search for the left / only camera, one for the right camera of a fisheye stereo frame); the
// "frame feature already matched" rule (:266-268) makes the loop sequential, so the queries are replayed in the reference's
// order and a query whose best or second-best candidate has been taken in the meantime is scanned again with the current matches.
int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches) {
  const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
  vpMapPointMatches = std::vector<MapPoint*>(F.N, static_cast<MapPoint*>(nullptr));
  const bool rig = F.Nleft != -1;
  // queries in visiting order, each with the frame-feature list of its node split by camera
  std::vector<int> qKF;
  std::vector<uint8_t> qdesc;
  std::vector<int32_t> offL(1, 0), idxL, offR(1, 0), idxR;
  for_each_common_node(pKF->mFeatVec, F.mFeatVec, [&](const std::vector<unsigned int>& featsKF, const std::vector<unsigned int>& featsF) {
    for (const unsigned int realIdxKF : featsKF) {
      MapPoint* pMP = vpMapPointsKF[realIdxKF];
      if (!pMP || pMP->isBad()) continue;
      qKF.push_back((int)realIdxKF);
      push_desc(qdesc, pKF->mDescriptors, (int)realIdxKF);
      for (const unsigned int iF : featsF) {
        if (!rig || (int)iF < F.Nleft) idxL.push_back((int32_t)iF); else idxR.push_back((int32_t)iF);
      }
      offL.push_back((int32_t)idxL.size()); offR.push_back((int32_t)idxR.size());
    }
  });
  const int nq = (int)qKF.size();
  if (nq == 0) return 0;
  Found foundL, foundR;
  if (!device_search_lists(qdesc, F.mDescriptors, F.N, offL, idxL, foundL)) return 0;
  if (rig && !device_search_lists(qdesc, F.mDescriptors, F.N, offR, idxR, foundR)) return 0;

  int nmatches = 0;
  RotHist hist;
  auto matched = [&vpMapPointMatches](int iF) { return vpMapPointMatches[iF] != nullptr; };   // any match blocks its feature (:266-268)
  auto histo = [&](int realIdxKF, int idxF) {
    // :333-345, 363-375 choose by the second camera's presence, and mvKeys where the frame has none: not keypoint_of()
    const cv::KeyPoint& kp = (!pKF->mpCamera2) ? pKF->mvKeysUn[realIdxKF]
                             : (realIdxKF >= pKF->NLeft) ? pKF->mvKeysRight[realIdxKF - pKF->NLeft] : pKF->mvKeys[realIdxKF];
    const cv::KeyPoint& Fkp = (!rig) ? F.mvKeys[idxF] : (idxF >= F.Nleft) ? F.mvKeysRight[idxF - F.Nleft] : F.mvKeys[idxF];
    hist.add(kp.angle, Fkp.angle, idxF);
  };
  for (int q = 0; q < nq; ++q) {
    MapPoint* pMP = vpMapPointsKF[qKF[q]];
    const Best2 bl = best_of_list(foundL, qdesc, F.mDescriptors, offL, idxL, q, kBestOrSecondTaken, matched);
    const Best2 br = rig ? best_of_list(foundR, qdesc, F.mDescriptors, offR, idxR, q, kBestOrSecondTaken, matched) : Best2();
    if (bl.dist <= TH_LOW) {
      if (static_cast<float>(bl.dist) < mfNNratio * static_cast<float>(bl.dist2)) {
        vpMapPointMatches[bl.idx] = pMP;
        if (mbCheckOrientation) histo(qKF[q], bl.idx);
        nmatches++;
      }
      if (br.dist <= TH_LOW) {   // the right-camera best is taken without a ratio test ("|| true", :352)
        vpMapPointMatches[br.idx] = pMP;
        if (mbCheckOrientation) histo(qKF[q], br.idx);
        nmatches++;
      }
    }
  }
  if (mbCheckOrientation) hist.prune([&](int idxF) { vpMapPointMatches[idxF] = static_cast<MapPoint*>(nullptr); nmatches--; });
  return nmatches;
}

// src/ORBmatcher.cc:765-905: same scheme as the keyframe / frame variant.  The static candidate filters (keyframe 2's feature holds a
// good map point, index below mvKeysUn.size() on a fisheye rig keyframe) are applied when the lists are built; vbMatched2 is the
// sequential part that the ordered replay reproduces.
int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12) {
  const std::vector<cv::KeyPoint>& vKeysUn1 = pKF1->mvKeysUn;
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  const std::vector<cv::KeyPoint>& vKeysUn2 = pKF2->mvKeysUn;
  const std::vector<MapPoint*> vpMapPoints2 = pKF2->GetMapPointMatches();
  vpMatches12 = std::vector<MapPoint*>(vpMapPoints1.size(), static_cast<MapPoint*>(nullptr));
  std::vector<bool> vbMatched2(vpMapPoints2.size(), false);
  std::vector<int> q1;
  std::vector<uint8_t> qdesc;
  std::vector<int32_t> off(1, 0), idx;
  for_each_common_node(pKF1->mFeatVec, pKF2->mFeatVec, [&](const std::vector<unsigned int>& feats1, const std::vector<unsigned int>& feats2) {
    for (const unsigned int idx1 : feats1) {
      if (pKF1->NLeft != -1 && idx1 >= pKF1->mvKeysUn.size()) continue;
      MapPoint* pMP1 = vpMapPoints1[idx1];
      if (!pMP1 || pMP1->isBad()) continue;
      q1.push_back((int)idx1);
      push_desc(qdesc, pKF1->mDescriptors, (int)idx1);
      for (const unsigned int idx2 : feats2) {
        if (pKF2->NLeft != -1 && idx2 >= pKF2->mvKeysUn.size()) continue;
        MapPoint* pMP2 = vpMapPoints2[idx2];
        if (!pMP2 || pMP2->isBad()) continue;
        idx.push_back((int32_t)idx2);
      }
      off.push_back((int32_t)idx.size());
    }
  });
  const int nq = (int)q1.size();
  if (nq == 0) return 0;
  Found found;
  if (!device_search_lists(qdesc, pKF2->mDescriptors, (int)vpMapPoints2.size(), off, idx, found)) return 0;
  RotHist hist;
  int nmatches = 0;
  for (int q = 0; q < nq; ++q) {
    const int idx1 = q1[q];
    const Best2 b = best_of_list(found, qdesc, pKF2->mDescriptors, off, idx, q, kBestOrSecondTaken, [&vbMatched2](int i2) { return (bool)vbMatched2[i2]; });
    if (b.dist < TH_LOW) {
      if (static_cast<float>(b.dist) < mfNNratio * static_cast<float>(b.dist2)) {
        vpMatches12[idx1] = vpMapPoints2[b.idx];
        vbMatched2[b.idx] = true;                                  // any match blocks its feature (:853)
        if (mbCheckOrientation) hist.add(vKeysUn1[idx1].angle, vKeysUn2[b.idx].angle, idx1);   // mvKeysUn on both sides whatever the layout (:857)
        nmatches++;
      }
    }
  }
  if (mbCheckOrientation) hist.prune([&](int idx1) { vpMatches12[idx1] = static_cast<MapPoint*>(nullptr); nmatches--; });
  return nmatches;
}

}  // namespace ORB_SLAM3
