// Frame.cc -- Frame::isInFrustum on the device (reference src/Frame.cc:513-587, Nleft == -1 branch) and
// Frame::UpdatePoseMatrices (src/Frame.cc:473-480).
//
// Tracking::SearchLocalPoints (src/Tracking.cc:3411-3432) calls isInFrustum once per local map point; the batch overload
// below projects the whole list in one launch of k_frustum (csrc/orb_device.hip) and writes the same MapPoint fields
// (mbTrackInView, mTrackProjX/Y/XR, mTrackDepth, mnTrackScaleLevel, mTrackViewCos).  The single-point overload keeps the
// reference signature and goes through the same kernel with a batch of one.  There is no CPU fallback.
//
// Frame::ComputeStereoMatches (src/Frame.cc:816-986, called by the stereo constructor at :141) is a pack and a write-back around
// osh_orb_stereo_match (csrc/stereo_device.hip): the row-band search, the SAD window, the parabola and the median cut run on the device.
//
// Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1131-1171, called by the rig constructor at :1110) is the same around
// osh_orb_fisheye_stereo_match (csrc/fisheye_stereo_device.hip): the 2-nearest-neighbour search, Lowe's test and
// KannalaBrandt8::TriangulateMatches run on the device.  mvuRight stays -1, as in the reference.
#include <cstdio>
#include <vector>
#include "Frame.h"
#include "MapPoint.h"
#include "host_pack.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // csrc/host/ORBmatcher.cc

void Frame::UpdatePoseMatrices() {
  const Sophus::SE3<float> Twc = mTcw.inverse();
  mRwc = Twc.rotationMatrix();
  mOw = Twc.translation();
  mRcw = mTcw.rotationMatrix();
  mtcw = mTcw.translation();
}

// src/Frame.cc:482-488 through the SE3 product Twc * Tcb (the stand-in Eigen types carry no matrix operators)
Eigen::Vector3f Frame::GetImuPosition() const { return (mTcw.inverse() * mImuCalib.mTcb).translation(); }
Eigen::Matrix3f Frame::GetImuRotation() { return (mTcw.inverse() * mImuCalib.mTcb).rotationMatrix(); }

// src/Frame.cc:458-471
void Frame::SetImuPoseVelocity(const Eigen::Matrix3f& Rwb, const Eigen::Vector3f& twb, const Eigen::Vector3f& Vwb) {
  mVw = Vwb;
  mbHasVelocity = true;
  const Sophus::SE3f Twb(Rwb, twb);
  mTcw = mImuCalib.mTcb * Twb.inverse();
  ++mnPoseSets;
  UpdatePoseMatrices();
}

int Frame::isInFrustum(const std::vector<MapPoint*>& vpMPs, float viewingCosLimit, std::vector<bool>& vbInView) {
  const int n = (int)vpMPs.size();
  vbInView.assign(n, false);
  if (n == 0) return 0;
  if (Nleft != -1 || mpCamera2) {
    std::fprintf(stderr, "Frame::isInFrustum: fisheye-stereo frames (Nleft != -1) are not supported by the MI355X path yet\n");
    return -1;
  }
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) return -1;
  osh_frustum_frame f;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) f.Rcw[3 * r + c] = mRcw(r, c);
    f.tcw[r] = mtcw(r); f.Ow[r] = mOw(r);
  }
  f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy; f.bf = mbf;
  f.min_x = mnMinX; f.max_x = mnMaxX; f.min_y = mnMinY; f.max_y = mnMaxY;
  f.log_scale_factor = mfLogScaleFactor; f.n_scale_levels = mnScaleLevels; f.viewing_cos_limit = viewingCosLimit;
  f.fisheye = (mpCamera && mpCamera->GetType() == GeometricCamera::CAM_FISHEYE) ? 1 : 0;   // mpCamera->project(Pc) (:532)
  for (int k = 0; k < 4; ++k) f.kb8[k] = f.fisheye ? mpCamera->getParameter(4 + k) : 0.f;
  std::vector<float> pos((size_t)n * 3), nrm((size_t)n * 3), dmin(n), dmax(n);
  for (int i = 0; i < n; ++i) {
    const Eigen::Vector3f P = vpMPs[i]->GetWorldPos(), Pn = vpMPs[i]->GetNormal();
    for (int k = 0; k < 3; ++k) { pos[3 * (size_t)i + k] = P(k); nrm[3 * (size_t)i + k] = Pn(k); }
    dmin[i] = vpMPs[i]->mfMinDistance; dmax[i] = vpMPs[i]->mfMaxDistance;
  }
  osh_frustum_points pts{n, pos.data(), nrm.data(), dmin.data(), dmax.data()};
  std::vector<uint8_t> stage(n);
  std::vector<float> px(n), py(n), pxr(n), depth(n), vcos(n);
  std::vector<int32_t> level(n);
  osh_frustum_result res{stage.data(), px.data(), py.data(), pxr.data(), depth.data(), vcos.data(), level.data()};
  if (osh_orb_frustum(ctx, &f, &pts, &res) != OSH_OK) {
    std::fprintf(stderr, "Frame::isInFrustum: %s\n", osh_last_error());
    return -1;
  }
  int n_in = 0;
  for (int i = 0; i < n; ++i) {
    MapPoint* pMP = vpMPs[i];
    pMP->mbTrackInView = false;                 // :515
    pMP->mTrackProjX = px[i];                   // -1 (:516-517) or uv (:539-540)
    pMP->mTrackProjY = py[i];
    if (stage[i] == 2) {                        // :563-571
      pMP->mbTrackInView = true;
      pMP->mTrackProjXR = pxr[i];
      pMP->mTrackDepth = depth[i];
      pMP->mnTrackScaleLevel = level[i];
      pMP->mTrackViewCos = vcos[i];
      vbInView[i] = true;
      ++n_in;
    }
  }
  return n_in;
}

void Frame::ComputeStereoMatches() {
  const size_t n = mvKeys.size();
  mvuRight = std::vector<float>(n, -1.0f);   // :818-819; the state in which every keypoint is monocular
  mvDepth = std::vector<float>(n, -1.0f);
  if (n == 0) return;
  StereoPack pk;
  if (!PackStereoMatches(*this, pk)) {
    std::fprintf(stderr, "Frame::ComputeStereoMatches: %s\n", pk.unsupported);
    return;
  }
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) {
    std::fprintf(stderr, "Frame::ComputeStereoMatches: %s\n", osh_last_error());
    return;
  }
  osh_stereo_frame f;
  pk.fill(f, *this);
  std::vector<float> u_right(n), depth(n);
  osh_stereo_result res{u_right.data(), depth.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
  if (osh_orb_stereo_match(ctx, 1, &f, &res) != OSH_OK) {
    std::fprintf(stderr, "Frame::ComputeStereoMatches: %s\n", osh_last_error());
    return;
  }
  mvuRight.swap(u_right);
  mvDepth.swap(depth);
}

void Frame::ExtractAndMatchStereo(const cv::Mat& imLeft, const cv::Mat& imRight, const ImagePrep* pPrepLeft, const ImagePrep* pPrepRight,
                                  std::vector<cv::Mat>* pvGray) {
  mvKeys.clear(); mvKeysRight.clear();
  mDescriptors.release(); mDescriptorsRight.release();
  mvuRight.clear(); mvDepth.clear();
  N = 0;
  if (pvGray) pvGray->clear();
  if (!mpORBextractorLeft || !mpORBextractorRight || (pPrepLeft == nullptr) != (pPrepRight == nullptr)) {
    std::fprintf(stderr, "Frame::ExtractAndMatchStereo: two extractors and an ImagePrep for both images or for none\n");
    return;
  }
  // the packing, the call and the write-back are ExtractBatchFrom's, with the match of the pair behind the two extractions
  const std::vector<ORBextractor*> extractors{mpORBextractorLeft, mpORBextractorRight};
  const std::vector<cv::Mat> images{imLeft, imRight};
  std::vector<ImagePrep> prep;
  if (pPrepLeft) prep = {*pPrepLeft, *pPrepRight};
  std::vector<std::vector<cv::KeyPoint> > keys;
  std::vector<cv::Mat> descriptors;
  const std::vector<std::vector<int> > lapping(2, std::vector<int>{0, 0});   // :118-119
  std::vector<int> mono;
  ORBextractor::StereoMatch stereo;
  stereo.bf = mbf; stereo.b = mb;
  ORBextractor::ExtractBatchFrom("ExtractAndMatchStereo", extractors, images, pPrepLeft ? &prep : nullptr, keys, descriptors, lapping, mono, false, pvGray, &stereo);
  if (!stereo.bOk || keys.size() != 2 || descriptors.size() != 2 || stereo.vuRight.size() != keys[0].size()) {
    if (pvGray) pvGray->clear();
    return;   // ExtractBatchFrom has said why
  }
  mvKeys.swap(keys[0]); mvKeysRight.swap(keys[1]);
  mDescriptors = descriptors[0]; mDescriptorsRight = descriptors[1];
  N = (int)mvKeys.size();                     // :132
  mvuRight.swap(stereo.vuRight);
  mvDepth.swap(stereo.vDepth);
}

void Frame::ComputeStereoFishEyeMatches() {
  const size_t nl = mvKeys.size(), nr = mvKeysRight.size();
  mvLeftToRightMatch = std::vector<int>(nl, -1);   // :1139-1144; the state in which every keypoint is unmatched
  mvRightToLeftMatch = std::vector<int>(nr, -1);
  mvDepth = std::vector<float>(nl, -1.0f);
  mvuRight = std::vector<float>(nl, -1);
  mvStereo3Dpoints = std::vector<Eigen::Vector3f>(nl);
  mnCloseMPs = 0;
  FisheyeStereoPack pk;
  if (!PackStereoFishEyeMatches(*this, pk)) {
    std::fprintf(stderr, "Frame::ComputeStereoFishEyeMatches: %s\n", pk.unsupported);
    return;
  }
  if (nl == 0 && nr == 0) return;
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) {
    std::fprintf(stderr, "Frame::ComputeStereoFishEyeMatches: %s\n", osh_last_error());
    return;
  }
  osh_fisheye_stereo_frame f;
  pk.fill(f, *this);
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) f.Rlr[3 * r + c] = mRlr(r, c); f.tlr[r] = mtlr(r); }   // private members
  std::vector<int32_t> l2r(nl), r2l(nr);
  std::vector<float> depth(nl), p3d(nl * 3);
  osh_fisheye_stereo_result res{l2r.data(), r2l.data(), depth.data(), p3d.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
  if (osh_orb_fisheye_stereo_match(ctx, 1, &f, &res) != OSH_OK) {
    std::fprintf(stderr, "Frame::ComputeStereoFishEyeMatches: %s\n", osh_last_error());
    return;
  }
  mvLeftToRightMatch.assign(l2r.begin(), l2r.end());
  mvRightToLeftMatch.assign(r2l.begin(), r2l.end());
  mvDepth.swap(depth);
  for (size_t i = 0; i < nl; ++i) mvStereo3Dpoints[i] = Eigen::Vector3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
}

bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit) {
  std::vector<bool> in;
  return isInFrustum(std::vector<MapPoint*>{pMP}, viewingCosLimit, in) == 1;
}

}  // namespace ORB_SLAM3
