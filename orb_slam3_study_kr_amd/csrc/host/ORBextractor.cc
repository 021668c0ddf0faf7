// ORBextractor.cc -- ORBextractor::ComputeKeyPointsOctTree (reference src/ORBextractor.cc:781-896) and ORBextractor::operator()
// (:1086-1168) on MI355X (host side).
//
// The loops over the cells of every level (:787-872: cv::FAST at iniThFAST, again at minThFAST for a cell without corners) are ONE
// osh_orb_fast_detect call for the whole pyramid (csrc/orb_fast_device.hip); DistributeOctTree stays the reference's and runs per
// level on what the device returned, followed by the write-back of :880-890; computeOrientation of all levels (:893-895) is ONE
// osh_orb_ic_angle call on the pyramid the detector left on the device.  In the integrator's tree the constructor and
// DistributeOctTree stay the reference's; these bodies replace :781-896, :1086-1168 and :1170-1195.  ComputeKeyPointsOctTree leaves
// the detector's pyramid token in the member mnPyramidToken.
//
// ComputePyramid (:1170-1195): the bordered `temp` of every level is allocated here and mvImagePyramid[level] is the view into it,
// as the reference leaves them; cv::resize and copyMakeBorder of all levels are ONE osh_orb_pyramid_build call
// (csrc/orb_pyramid_device.hip) that keeps the levels on the device and downloads them with their borders.  Its token goes into the
// member mnBuiltPyramidToken; ComputeKeyPointsOctTree consumes it and, if it is still valid, detects on the resident levels with
// osh_orb_fast_detect_resident instead of uploading mvImagePyramid (so an edit of mvImagePyramid between the two calls is not seen
// by the detector).  With the member 0, or a stale token, it does what it did before.
//
// operator(): ComputePyramid, ComputeKeyPointsOctTree, then the per-level GaussianBlur and computeDescriptors of :1123-1140 as ONE
// osh_orb_describe call for all levels (csrc/orb_brief_device.hip) on the pyramid the detector left on the device (or on
// mvImagePyramid itself when there is no token), with the member `pattern` as the sampling table; the write-back of :1143-1164
// follows on the host.
//
// Deviations from the reference, all intended:
//   * a level with fewer than 35 columns or rows between its borders has no cells (the reference divides by zero there);
//   * fastAtan2 is OpenCV's documented scalar form in unfused float32 operations (include/orbslam3_hip.h);
//   * on a device error, or a pyramid the call refuses, a message goes to stderr and allKeypoints is empty at every level;
//   * ComputePyramid: the resampling is the one include/orbslam3_hip.h defines (parity with cv::resize is not pinned); on a device
//     error or a refused call a message goes to stderr and every level of mvImagePyramid is empty;
//   * operator(): cos and sin of the keypoint angle through the FP64 functions, the sample offsets in unfused float32, the blur as
//     include/orbslam3_hip.h defines it (parity with cv::GaussianBlur is not pinned); on a device error or a refused call a message
//     goes to stderr and the result is no keypoints (return value 0, descriptors released).
//
// ExtractBatch (a member to ADD): operator() of several extractors, for example the left and the right one of a stereo frame, as ONE
// osh_orb_extract call (csrc/orb_extract_device.hip): pyramid, detector, quadtree, orientation, blur and descriptors on the device
// with no keypoint array crossing to the host in between, then the write-back of :1143-1164 per extractor.  Its quadtree is the rule
// of include/orbslam3_hip.h (DistributeOctTreeDevice's), not DistributeOctTree.  An empty image gives -1 for that extractor; a device
// error or a refused call gives a message on stderr and no keypoints for any extractor.
//
// ExtractBatchRaw (a member to ADD): ExtractBatch on the camera images as they arrive, as ONE osh_orb_extract_raw call
// (csrc/orb_prepare_device.hip): per image an ImagePrep (include/RectifyMap.h) says how the grey level-0 image is made on the device
// (the cv::remap or cv::resize of System::Track* on every channel, then the cvtColor of Tracking::GrabImage*, as
// include/orbslam3_hip.h defines them; parity with OpenCV is not pinned).  The two share one body, ExtractBatchFrom; the write-back,
// mvImagePyramid, mnPyramidToken, the -1 of an empty image and the error behaviour are ExtractBatch's.
//
// DistributeOctTreeDevice (a member to ADD; :480-779): the arguments and the result of DistributeOctTree, the selection as ONE
// osh_orb_octree_distribute call (csrc/orb_octree_device.hip) under the rule include/orbslam3_hip.h states.  Nothing calls it here:
// ComputeKeyPointsOctTree keeps the reference's DistributeOctTree, an integrator opts in.  Its deviations from the reference's list
// code (the stable sort, nIni == 0, a root index equal to nIni) are those of the rule; candidates the call refuses as invalid (not
// finite, x outside [0, maxX - minX), negative y, an empty area) give a message on stderr and no keypoints.
//
// What more than one body needs is stated once: the size of a level, `pattern` as the table of the calls and the write-back of
// :1143-1164 in csrc/host/orb_extract_steps.h (no device call; it goes into the integrator's tree with this file), the bordered
// levels, a cv::Mat as an image of the calls and the messages that carry osh_last_error() in the helpers below.
#include "ORBextractor.h"

#include <algorithm>
#include <cstdio>
#include <vector>

#include "orb_extract_steps.h"
#include "orbslam3_hip.h"
#include "../orb_octree.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // csrc/host/ORBmatcher.cc
int HostMatcherDevice();

// "ORBextractor::<who>: <what><then>" on stderr; `what` is the reason of the call that was just refused unless the caller has its own
static void Report(const char* who, const char* what = osh_last_error(), const char* then = "") {
  std::fprintf(stderr, "ORBextractor::%s: %s%s\n", who, what, then);
}

// This thread's context; null: reported under `who`
static osh_orb_ctx* Context(const char* who) {
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) Report(who);
  return ctx;
}

// A cv::Mat as an osh_stereo_image or osh_pyramid_image: in place, a view into a bordered image with that image's stride
template <class Image>
static Image ImageOf(const cv::Mat& im) {
  Image image{};
  image.data = im.empty() ? nullptr : const_cast<uint8_t*>(im.ptr<uint8_t>(0));
  image.rows = im.rows; image.cols = im.cols; image.stride = (int64_t)(size_t)im.step;
  return image;
}

// The levels of mvImagePyramid as the calls read them
static std::vector<osh_stereo_image> PyramidViews(const std::vector<cv::Mat>& levels, int nlevels) {
  std::vector<osh_stereo_image> pyramid(nlevels);
  for (int level = 0; level < nlevels; ++level) pyramid[level] = ImageOf<osh_stereo_image>(levels[level]);
  return pyramid;
}

// :1174-1178 per level: the bordered `temp` is allocated and levels[level] is the view into it, as the reference leaves
// mvImagePyramid[level]; out[level] is where a call writes that level.  Returns the first level that has no pixels or too many,
// nlevels when there is none
static int BorderedLevels(int rows, int cols, const std::vector<float>& invScale, int nlevels, std::vector<cv::Mat>& levels,
                          std::vector<osh_pyramid_image>& out) {
  levels.resize(nlevels); out.resize(nlevels);
  for (int level = 0; level < nlevels; ++level) {
    int h, w;
    if (!LevelShape(rows, cols, invScale[level], h, w)) return level;
    cv::Mat temp(h + 2 * kEdge, w + 2 * kEdge);
    levels[level] = temp.view(kEdge, kEdge, h, w);
    out[level] = ImageOf<osh_pyramid_image>(levels[level]);
  }
  return nlevels;
}

// The `total` keypoints of allKeypoints, level after level, as the arrays of one call; `angle` may be null
static void FlattenKeypoints(const std::vector<std::vector<cv::KeyPoint> >& allKeypoints, int nlevels, size_t total, std::vector<float>& pts,
                             std::vector<int32_t>& lvl, std::vector<float>* angle) {
  pts.resize(total * 2); lvl.resize(total);
  if (angle) angle->resize(total);
  size_t n = 0;
  for (int l = 0; l < nlevels; ++l)
    for (const cv::KeyPoint& kp : allKeypoints[l]) {
      pts[2 * n] = kp.pt.x; pts[2 * n + 1] = kp.pt.y; lvl[n] = l;
      if (angle) (*angle)[n] = kp.angle;
      ++n;
    }
}

// By token while there is one; on a refused token (stale: another extractor used this thread's context in between) or without
// one, with the pyramid itself.  False: that call was refused too
template <class ByToken, class ByPyramid>
static bool ByTokenOrPyramid(bool& have_token, ByToken by_token, ByPyramid by_pyramid) {
  if (have_token && by_token() == OSH_OK) return true;
  have_token = false;
  return by_pyramid() == OSH_OK;
}

void ORBextractor::ComputePyramid(cv::Mat image) {
  mnBuiltPyramidToken = 0;
  mvImagePyramid.assign(nlevels > 0 ? nlevels : 0, cv::Mat());
  if (nlevels <= 0 || image.empty()) return;
  if ((int)mvInvScaleFactor.size() < nlevels) {
    std::fprintf(stderr, "ORBextractor::ComputePyramid: mvInvScaleFactor has %d of %d entries\n", (int)mvInvScaleFactor.size(), nlevels);
    return;
  }
  std::vector<cv::Mat> levels;
  std::vector<osh_pyramid_image> out;
  const int bad = BorderedLevels(image.rows, image.cols, mvInvScaleFactor, nlevels, levels, out);
  if (bad < nlevels) { std::fprintf(stderr, "ORBextractor::ComputePyramid: level %d has no pixels or too many\n", bad); return; }
  osh_orb_ctx* ctx = Context("ComputePyramid");
  if (!ctx) return;
  // the resize and copyMakeBorder of every level (:1181-1193) in one call; the levels stay on the device under the token
  const osh_pyramid_frame frame{ImageOf<osh_stereo_image>(image), nlevels, mvInvScaleFactor.data()};
  osh_pyramid_result res{};
  res.levels = out.data(); res.border = kEdge;
  if (osh_orb_pyramid_build(ctx, 1, &frame, &res) != OSH_OK) return Report("ComputePyramid");
  mvImagePyramid = levels;
  mnBuiltPyramidToken = res.pyramid_token;
}

void ORBextractor::ComputeKeyPointsOctTree(std::vector<std::vector<cv::KeyPoint> >& allKeypoints) {
  allKeypoints.clear();
  allKeypoints.resize(nlevels);
  mnPyramidToken = 0;
  const uint64_t built = mnBuiltPyramidToken;   // consumed: a later call on a hand-set pyramid must not see it
  mnBuiltPyramidToken = 0;
  if (nlevels <= 0) return;
  if ((int)mvImagePyramid.size() < nlevels) {
    std::fprintf(stderr, "ORBextractor::ComputeKeyPointsOctTree: the pyramid has %d of %d levels\n", (int)mvImagePyramid.size(), nlevels);
    return;
  }
  osh_orb_ctx* ctx = Context("ComputeKeyPointsOctTree");
  if (!ctx) return;

  // every cell of every level (:787-872) in one call
  const std::vector<osh_stereo_image> pyramid = PyramidViews(mvImagePyramid, nlevels);
  const osh_fast_frame frame{nlevels, pyramid.data(), iniThFAST, minThFAST};
  std::vector<int32_t> levelCount(nlevels);
  std::vector<float> xy, response;
  osh_fast_result res{};
  res.level_count = levelCount.data();
  size_t capacity = (size_t)(nfeatures > 0 ? nfeatures : 0) * 10 * (size_t)nlevels;   // vToDistributeKeys.reserve(nfeatures*10) per level
  // the pyramid ComputePyramid left on the device, if it is still there (another extractor may have used this thread's context in
  // between: a stale token is refused and the levels of mvImagePyramid go up instead)
  const osh_fast_resident_frame resident{built, iniThFAST, minThFAST};
  bool use_resident = built != 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    xy.resize(capacity * 2); response.resize(capacity);
    res.capacity = (int32_t)capacity; res.xy = xy.data(); res.response = response.data();
    if (!ByTokenOrPyramid(use_resident, [&] { return osh_orb_fast_detect_resident(ctx, 1, &resident, &res); }, [&] { return osh_orb_fast_detect(ctx, 1, &frame, &res); }))
      return Report("ComputeKeyPointsOctTree");
    if ((size_t)res.n_out <= capacity) break;
    capacity = (size_t)res.n_out;   // the counts came back without the arrays: once more with room for them
  }

  // per level: the candidates of the device as the octree's input, the reference's DistributeOctTree, and what :880-890 add to its
  // selection (the border, the level, the patch diameter 31 at the level's scale, cut to int)
  constexpr int kBorder = 16;   // EDGE_THRESHOLD - 3, the margin of the detect area on every side
  size_t offset = 0, total = 0;
  for (int l = 0; l < nlevels; ++l) {
    std::vector<cv::KeyPoint> candidates((size_t)levelCount[l]);
    for (cv::KeyPoint& c : candidates) {   // the fields cv::FAST fills: size 7, no angle, the score as response
      c.pt.x = xy[2 * offset]; c.pt.y = xy[2 * offset + 1]; c.response = response[offset];
      c.size = 7.f; c.angle = -1.f; c.octave = 0; c.class_id = -1;
      ++offset;
    }
    allKeypoints[l] = DistributeOctTree(candidates, kBorder, mvImagePyramid[l].cols - kBorder, kBorder, mvImagePyramid[l].rows - kBorder,
                                        mnFeaturesPerLevel[l], l);
    const float diameter = (float)(int)(31 * mvScaleFactor[l]);
    for (cv::KeyPoint& kp : allKeypoints[l]) {
      kp.pt.x += kBorder; kp.pt.y += kBorder;
      kp.octave = l;
      kp.size = diameter;
    }
    total += allKeypoints[l].size();
  }

  // the orientation of every kept keypoint (:893-895): all levels in one call, on the pyramid the detector left on the device
  if (total == 0) return;
  std::vector<float> pts, angle(total);
  std::vector<int32_t> lvl;
  FlattenKeypoints(allKeypoints, nlevels, total, pts, lvl, nullptr);
  const osh_ic_angle_frame icf{0, nullptr, res.pyramid_token, (int32_t)total, pts.data(), lvl.data()};
  const osh_ic_angle_result icr{angle.data(), nullptr, nullptr};
  if (osh_orb_ic_angle(ctx, 1, &icf, &icr) != OSH_OK) {
    Report("ComputeKeyPointsOctTree");
    for (std::vector<cv::KeyPoint>& kps : allKeypoints) kps.clear();
    return;
  }
  size_t n = 0;
  for (std::vector<cv::KeyPoint>& kps : allKeypoints)
    for (cv::KeyPoint& kp : kps) kp.angle = angle[n++];
  mnPyramidToken = res.pyramid_token;
}

std::vector<cv::KeyPoint> ORBextractor::DistributeOctTreeDevice(const std::vector<cv::KeyPoint>& vToDistributeKeys, const int& minX, const int& maxX,
                                                                const int& minY, const int& maxY, const int& N, const int& /*level*/) {
  std::vector<cv::KeyPoint> vResultKeys;
  const int n = (int)vToDistributeKeys.size(), W = maxX - minX, H = maxY - minY;
  std::vector<float> xy((size_t)n * 2), response(n);
  for (int k = 0; k < n; ++k) { xy[2 * k] = vToDistributeKeys[k].pt.x; xy[2 * k + 1] = vToDistributeKeys[k].pt.y; response[k] = vToDistributeKeys[k].response; }
  const char* why = "";
  const int valid = osh::oct_validate_list(n, xy.data(), response.data(), W, H, N, &why);
  if (valid == osh::kOctInvalid) {
    Report("DistributeOctTreeDevice", why);
    return vResultKeys;
  }
  std::vector<int32_t> index(n);   // a node keeps one of its keys: never more than n
  int kept = -1;
  if (valid != osh::kOctOk) {
    Report("DistributeOctTreeDevice", why, ": on the host");
  } else {
    const osh_octree_list list{n, xy.data(), response.data(), W, H, N};
    osh_octree_result res{n, 0, 0, index.data()};
    osh_orb_ctx* ctx = HostMatcherContext();
    if (ctx && osh_orb_octree_distribute(ctx, 1, &list, &res) == OSH_OK) kept = res.n_out;
    else Report("DistributeOctTreeDevice", osh_last_error(), ": on the host");
  }
  if (kept < 0) {
    std::vector<int> host;
    if (osh::octree_distribute_host(n, xy.data(), response.data(), W, H, N, host) != osh::kOctOk) return vResultKeys;
    kept = (int)host.size();
    std::copy(host.begin(), host.end(), index.begin());
  }
  vResultKeys.reserve(kept);
  for (int i = 0; i < kept; ++i) vResultKeys.push_back(vToDistributeKeys[index[i]]);
  return vResultKeys;
}

void ORBextractor::ExtractBatch(const std::vector<ORBextractor*>& vpExtractors, const std::vector<cv::Mat>& vImages,
                                std::vector<std::vector<cv::KeyPoint> >& vKeypoints, std::vector<cv::Mat>& vDescriptors,
                                const std::vector<std::vector<int> >& vLappingAreas, std::vector<int>& vMonoIndex, bool bKeepPyramid) {
  ExtractBatchFrom("ExtractBatch", vpExtractors, vImages, nullptr, vKeypoints, vDescriptors, vLappingAreas, vMonoIndex, bKeepPyramid, nullptr);
}

void ORBextractor::ExtractBatchRaw(const std::vector<ORBextractor*>& vpExtractors, const std::vector<cv::Mat>& vRawImages,
                                   const std::vector<ImagePrep>& vPrep, std::vector<std::vector<cv::KeyPoint> >& vKeypoints,
                                   std::vector<cv::Mat>& vDescriptors, const std::vector<std::vector<int> >& vLappingAreas,
                                   std::vector<int>& vMonoIndex, bool bKeepPyramid, std::vector<cv::Mat>* pvGray) {
  ExtractBatchFrom("ExtractBatchRaw", vpExtractors, vRawImages, &vPrep, vKeypoints, vDescriptors, vLappingAreas, vMonoIndex, bKeepPyramid, pvGray);
}

// pvPrep null: vImages are grey and go up as they are (osh_orb_extract); else they are raw and level 0 is made on the device
// (osh_orb_extract_raw)
void ORBextractor::ExtractBatchFrom(const char* who, const std::vector<ORBextractor*>& vpExtractors, const std::vector<cv::Mat>& vImages,
                                    const std::vector<ImagePrep>* pvPrep, std::vector<std::vector<cv::KeyPoint> >& vKeypoints,
                                    std::vector<cv::Mat>& vDescriptors, const std::vector<std::vector<int> >& vLappingAreas,
                                    std::vector<int>& vMonoIndex, bool bKeepPyramid, std::vector<cv::Mat>* pvGray, StereoMatch* pStereo) {
  const size_t nExtractors = vpExtractors.size();
  if (pStereo) { pStereo->bOk = false; pStereo->vuRight.clear(); pStereo->vDepth.clear(); }
  vKeypoints.resize(nExtractors);
  vDescriptors.resize(nExtractors);
  vMonoIndex.assign(nExtractors, 0);
  if (pvGray) pvGray->assign(nExtractors, cv::Mat());
  if (vImages.size() != nExtractors || vLappingAreas.size() != nExtractors || (pvPrep && pvPrep->size() != nExtractors)) {
    std::fprintf(stderr, "ORBextractor::%s: %d extractors, %d images, %d lapping areas%s\n", who, (int)nExtractors, (int)vImages.size(), (int)vLappingAreas.size(),
                 pvPrep && pvPrep->size() != nExtractors ? ", another number of ImagePrep" : "");
    return;
  }
  // one frame of the call per extractor with an image; everything a frame points to lives in `job` until the call returns
  struct Job {
    size_t extractor;
    std::vector<cv::Mat> levels;
    std::vector<osh_pyramid_image> out;
    std::vector<int8_t> table;
    int rows, cols;   // of the grey image that is extracted
    cv::Mat gray;
    std::vector<int32_t> levelCount, level;
    std::vector<float> xy, response, angle, size;
    std::vector<uint8_t> desc;
  };
  std::vector<Job> jobs;
  bool ok = true;
  // osh_orb_extract_stereo hands no prepared image back: a caller that keeps the grey images gets them as the level 0 of the
  // downloaded levels, and pays for that download
  const bool bGrayFromLevels = pStereo && pvPrep && pvGray;
  const bool bLevels = bKeepPyramid || bGrayFromLevels;
  for (size_t i = 0; i < nExtractors; ++i) {
    ORBextractor* ex = vpExtractors[i];
    if (vImages[i].empty()) { vMonoIndex[i] = -1; continue; }   // operator() returns before it touches anything
    vKeypoints[i].clear();
    vDescriptors[i].release();
    ex->mnPyramidToken = ex->mnBuiltPyramidToken = 0;
    ex->mvImagePyramid.assign(ex->nlevels > 0 ? ex->nlevels : 0, cv::Mat());
    const int nl = ex->nlevels;
    if (nl <= 0 || (int)ex->mvInvScaleFactor.size() < nl || (int)ex->mvScaleFactor.size() < nl || (int)ex->mnFeaturesPerLevel.size() < nl ||
        ex->pattern.size() != 512 || vLappingAreas[i].size() < 2) {
      std::fprintf(stderr, "ORBextractor::%s: extractor %d: its level tables, its pattern or its lapping area do not fit\n", who, (int)i);
      ok = false;
      continue;
    }
    jobs.emplace_back();
    Job& j = jobs.back();
    j.extractor = i;
    j.table.resize(1024);
    if (!PatternTable(ex->pattern.data(), j.table.data())) ok = false;
    j.rows = vImages[i].rows; j.cols = vImages[i].cols;
    if (pvPrep) {
      const ImagePrep& prep = (*pvPrep)[i];
      PreparedShape(vImages[i].rows, vImages[i].cols, prep.pMap ? prep.pMap->rows() : 0, prep.pMap ? prep.pMap->cols() : 0, prep.newRows, prep.newCols, j.rows, j.cols);
      if (pvGray && j.rows > 0 && j.cols > 0 && j.rows <= OSH_FAST_MAX_SIDE && j.cols <= OSH_FAST_MAX_SIDE) j.gray = cv::Mat(j.rows, j.cols);
    }
    size_t capacity = 0;   // the quadtree keeps at most max(N + 3, 4 nIni) keypoints of a level, nIni <= OSH_OCTREE_MAX_ROOTS
    for (int l = 0; l < nl; ++l) capacity += (size_t)std::max(std::max(ex->mnFeaturesPerLevel[l], 0) + 3, 4 * OSH_OCTREE_MAX_ROOTS);
    j.levelCount.resize(nl); j.level.resize(capacity); j.xy.resize(capacity * 2); j.response.resize(capacity); j.angle.resize(capacity);
    j.size.resize(capacity); j.desc.resize(capacity * 32);
    if (bLevels) {   // the levels as ComputePyramid leaves them
      const int bad = BorderedLevels(j.rows, j.cols, ex->mvInvScaleFactor, nl, j.levels, j.out);
      if (bad < nl) { std::fprintf(stderr, "ORBextractor::%s: extractor %d: level %d has no pixels or too many\n", who, (int)i, bad); ok = false; }
    }
  }
  if (!ok) std::fprintf(stderr, "ORBextractor::%s: nothing extracted\n", who);
  if (ok && pStereo && (nExtractors != 2 || jobs.size() != 2)) {
    std::fprintf(stderr, "ORBextractor::%s: a stereo frame is two extractors with an image each, not %d with %d\n", who, (int)nExtractors, (int)jobs.size());
    return;
  }
  if (!ok || jobs.empty()) return;
  osh_orb_ctx* ctx = Context(who);
  if (!ctx) return;
  std::vector<osh_extract_frame> frames(jobs.size());
  std::vector<osh_extract_result> results(jobs.size());
  std::vector<osh_prepare_frame> rawFrames(pvPrep ? jobs.size() : 0);
  std::vector<osh_prepare_result> rawResults(pvPrep ? jobs.size() : 0);
  for (size_t k = 0; k < jobs.size(); ++k) {
    Job& j = jobs[k];
    const ORBextractor* ex = vpExtractors[j.extractor];
    osh_extract_frame& f = frames[k];
    if (pvPrep) {   // the raw image goes up; the frame of the extraction names the prepared size and brings no pixels
      const ImagePrep& prep = (*pvPrep)[j.extractor];
      const cv::Mat& raw = vImages[j.extractor];
      osh_prepare_frame& p = rawFrames[k];
      p = osh_prepare_frame{};
      p.image.data = raw.ptr<uint8_t>(0); p.image.rows = raw.rows; p.image.cols = raw.cols; p.image.stride = (int64_t)(size_t)raw.step;
      p.image.channels = raw.channels();
      p.order = prep.bRGB ? OSH_PREP_RGB : OSH_PREP_BGR;
      p.out_rows = prep.newRows; p.out_cols = prep.newCols;
      if (prep.pMap && !(p.map = prep.pMap->OnDevice(HostMatcherDevice()))) return Report(who);
      rawResults[k] = osh_prepare_result{};
      if (!j.gray.empty()) { rawResults[k].gray = j.gray.ptr<uint8_t>(0); rawResults[k].gray_stride = (int64_t)(size_t)j.gray.step; }
      f.image = osh_stereo_image{nullptr, j.rows, j.cols, (int64_t)j.cols};
    } else {
      f.image = ImageOf<osh_stereo_image>(vImages[j.extractor]);
    }
    f.n_levels = ex->nlevels; f.inv_scale = ex->mvInvScaleFactor.data(); f.scale = ex->mvScaleFactor.data();
    f.ini_th = ex->iniThFAST; f.min_th = ex->minThFAST; f.n_features = ex->mnFeaturesPerLevel.data();
    f.pattern = j.table.data(); f.blur_q8 = nullptr;
    osh_extract_result& r = results[k];
    r = osh_extract_result{};
    r.capacity = (int32_t)j.response.size(); r.level_count = j.levelCount.data(); r.xy = j.xy.data(); r.level = j.level.data();
    r.response = j.response.data(); r.angle = j.angle.data(); r.size = j.size.data(); r.descriptors = j.desc.data();
    r.levels = bLevels ? j.out.data() : nullptr; r.border = kEdge;
  }
  int rc;
  if (pStereo) {   // the two extractions and the match of the left keypoints against the right ones in one call
    pStereo->vuRight.resize(jobs[0].response.size()); pStereo->vDepth.resize(jobs[0].response.size());
    const osh_stereo_pair pair{pStereo->bf, pStereo->b};
    const osh_stereo_result matched{pStereo->vuRight.data(), pStereo->vDepth.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
    rc = osh_orb_extract_stereo(ctx, 1, pvPrep ? rawFrames.data() : nullptr, frames.data(), &pair, results.data(), &matched);
    for (size_t k = 0; rc == OSH_OK && bGrayFromLevels && k < jobs.size(); ++k) {
      Job& j = jobs[k];
      for (int r = 0; !j.gray.empty() && !j.levels.empty() && r < j.rows; ++r) std::memcpy(j.gray.ptr<uint8_t>(r), j.levels[0].ptr<uint8_t>(r), (size_t)j.cols);
    }
  } else {
    rc = pvPrep ? osh_orb_extract_raw(ctx, (int32_t)jobs.size(), rawFrames.data(), frames.data(), results.data(), rawResults.data())
                : osh_orb_extract(ctx, (int32_t)jobs.size(), frames.data(), results.data());
  }
  if (rc != OSH_OK) {
    if (pStereo) { pStereo->vuRight.clear(); pStereo->vDepth.clear(); }
    return Report(who);
  }
  if (pStereo) {
    pStereo->bOk = results[0].n_out <= results[0].capacity && results[1].n_out <= results[1].capacity;
    pStereo->vuRight.resize(pStereo->bOk ? (size_t)results[0].n_out : 0); pStereo->vDepth.resize(pStereo->vuRight.size());
  }
  for (size_t k = 0; k < jobs.size(); ++k) {
    const Job& j = jobs[k];
    ORBextractor* ex = vpExtractors[j.extractor];
    const osh_extract_result& r = results[k];
    if (pvGray) (*pvGray)[j.extractor] = j.gray;
    if (r.n_out > r.capacity) { std::fprintf(stderr, "ORBextractor::%s: extractor %d: %d keypoints for %d places\n", who, (int)j.extractor, r.n_out, r.capacity); continue; }
    if (bKeepPyramid) ex->mvImagePyramid = j.levels;
    ex->mnPyramidToken = r.pyramid_token;
    const int nkeypoints = r.n_out;
    std::vector<cv::KeyPoint>& keypoints = vKeypoints[j.extractor];
    cv::Mat& descriptors = vDescriptors[j.extractor];
    keypoints = std::vector<cv::KeyPoint>(nkeypoints);
    if (nkeypoints) descriptors.create(nkeypoints, 32, CV_8U);
    WriteBack<cv::KeyPoint> place(nkeypoints, ex->mvScaleFactor.data(), vLappingAreas[j.extractor].data(), keypoints.data(),
                                  nkeypoints ? descriptors.ptr<uint8_t>(0) : nullptr, (size_t)descriptors.step);
    for (int i = 0; i < nkeypoints; ++i) {
      cv::KeyPoint keypoint;
      keypoint.pt.x = j.xy[2 * i]; keypoint.pt.y = j.xy[2 * i + 1]; keypoint.response = j.response[i]; keypoint.angle = j.angle[i];
      keypoint.size = j.size[i]; keypoint.octave = j.level[i]; keypoint.class_id = -1;
      place(keypoint, &j.desc[32 * (size_t)i]);
    }
    vMonoIndex[j.extractor] = place.monoIndex;
  }
}

int ORBextractor::operator()(cv::InputArray _image, cv::InputArray /*_mask*/, std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors,
                             std::vector<int>& vLappingArea) {
  if (_image.empty()) return -1;
  cv::Mat image = _image.getMat();
  ComputePyramid(image);
  std::vector<std::vector<cv::KeyPoint> > allKeypoints;
  ComputeKeyPointsOctTree(allKeypoints);

  int nkeypoints = 0;
  for (int level = 0; level < nlevels; ++level) nkeypoints += (int)allKeypoints[level].size();

  // blur and descriptors of all levels (:1131-1138) in one call, in allKeypoints order
  std::vector<uint8_t> desc((size_t)nkeypoints * 32);
  if (nkeypoints) {
    bool ok = pattern.size() == 512 && (int)vLappingArea.size() >= 2;
    if (!ok) std::fprintf(stderr, "ORBextractor::operator(): the pattern has %d of 512 points or vLappingArea fewer than 2 entries\n", (int)pattern.size());
    osh_orb_ctx* ctx = ok ? Context("operator()") : nullptr;
    if (ctx) {
      std::vector<float> pts, angle;
      std::vector<int32_t> lvl;
      int8_t table[1024];
      ok = PatternTable(pattern.data(), table);
      if (!ok) std::fprintf(stderr, "ORBextractor::operator(): a pattern point does not fit 8 bits\n");
      FlattenKeypoints(allKeypoints, nlevels, (size_t)nkeypoints, pts, lvl, &angle);
      const std::vector<osh_stereo_image> pyramid = PyramidViews(mvImagePyramid, nlevels);
      osh_describe_frame named{};   // the keypoints on the resident pyramid; `brought`: on the levels of mvImagePyramid
      named.pyramid_token = mnPyramidToken;
      named.n = nkeypoints; named.xy = pts.data(); named.level = lvl.data(); named.angle = angle.data(); named.pattern = table; named.blur_q8 = nullptr;
      osh_describe_frame brought = named;
      brought.pyramid_token = 0; brought.n_levels = nlevels; brought.pyramid = pyramid.data();
      const osh_describe_result r{desc.data(), nullptr, nullptr};
      bool have_token = mnPyramidToken != 0;
      if (ok && !ByTokenOrPyramid(have_token, [&] { return osh_orb_describe(ctx, 1, &named, &r); }, [&] { return osh_orb_describe(ctx, 1, &brought, &r); })) {
        ok = false;
        Report("operator()");
      }
    }
    if (!ok || !ctx) { nkeypoints = 0; for (std::vector<cv::KeyPoint>& kps : allKeypoints) kps.clear(); }
  }

  cv::Mat descriptors;
  if (nkeypoints == 0) _descriptors.release();
  else { _descriptors.create(nkeypoints, 32, CV_8U); descriptors = _descriptors.getMat(); }
  _keypoints = std::vector<cv::KeyPoint>(nkeypoints);

  // ComputeKeyPointsOctTree left the level of every keypoint in its `octave`
  WriteBack<cv::KeyPoint> place(nkeypoints, mvScaleFactor.data(), vLappingArea.data(), _keypoints.data(), nkeypoints ? descriptors.ptr<uint8_t>(0) : nullptr,
                                (size_t)descriptors.step);
  size_t i = 0;
  for (const std::vector<cv::KeyPoint>& kps : allKeypoints)
    for (const cv::KeyPoint& keypoint : kps) place(keypoint, &desc[32 * i++]);
  return place.monoIndex;
}

}  // namespace ORB_SLAM3
