// prepare.cc -- csrc/orb_prepare.h (the statements k_prepare of csrc/orb_prepare_device.hip runs) on the host in one thread:
// osh_host_orb_prepare_cpu of include/orbslam3_hip_host.h, the CPU side of tests/test_prepare_cpu.py and the CPU baseline of
// profiles/prepare_timing.py (a rectify map is a host descriptor there: a resident one needs a device), and
// osh_host_orbextractor_extract_batch_raw, ORBextractor::ExtractBatchRaw of stand-in extractors with a RectifyMap per image.  Test
// library only.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "Frame.h"
#include "ORBextractor.h"
#include "RectifyMap.h"
#include "orbextractor_io.h"
#include "../orb_prepare.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

using namespace ORB_SLAM3;

extern "C" int osh_host_orbextractor_extract_batch_raw(int32_t n, const osh_host_extract_input* in, const osh_host_raw_image* raw,
                                                       const osh_host_extract_output* out, int32_t keep_pyramid, uint64_t* tokens, uint8_t* const* gray,
                                                       const int32_t* gray_capacity, int32_t* gray_rows, int32_t* gray_cols) {
  if (n < 0 || (n && (!in || !raw || !out || !tokens)) || (gray && (!gray_capacity || !gray_rows || !gray_cols))) return -1;
  std::vector<Standin> standins;
  standins.reserve((size_t)(n > 0 ? n : 0));   // the extractors stay where they are
  std::vector<cv::Mat> images;
  std::vector<std::unique_ptr<RectifyMap> > maps;
  std::vector<ImagePrep> prep;
  for (int i = 0; i < n; ++i) {
    const osh_host_raw_image& a = raw[i];
    const osh_host_extract_output& o = out[i];
    if (in[i].nlevels < 1 || a.rows < 0 || a.cols < 0 || a.channels < 1 || (a.rows && a.cols && !a.pixels) || (a.map_x && (!a.map_y || a.map_rows <= 0 || a.map_cols <= 0)) ||
        !o.level_rows || !o.level_cols || !o.ret || !o.desc_rows || !o.pixels_needed || o.capacity < 0 || o.pixel_capacity < 0) return -1;
    osh_host_extract_input extractor = in[i];
    extractor.rows = extractor.cols = 0;   // the stand-in's own image stays empty
    standins.emplace_back(extractor);
    cv::Mat image;
    if (a.rows && a.cols) {
      image = cv::Mat(a.rows, a.cols, a.channels);
      std::memcpy(image.ptr<uint8_t>(0), a.pixels, (size_t)a.rows * a.cols * a.channels);
    }
    images.push_back(image);
    ImagePrep p;
    p.bRGB = a.rgb != 0; p.newRows = a.new_rows; p.newCols = a.new_cols;
    if (a.map_x) {
      const size_t step = sizeof(float) * (size_t)a.map_cols;
      maps.emplace_back(new RectifyMap(a.map_x, step, a.map_y, step, a.map_rows, a.map_cols, a.rows, a.cols));
      p.pMap = maps.back().get();
    }
    prep.push_back(p);
  }
  std::vector<ORBextractor*> extractors;
  std::vector<std::vector<int> > lapping;
  for (Standin& s : standins) { extractors.push_back(&s.ex); lapping.push_back(s.lapping); }
  std::vector<std::vector<cv::KeyPoint> > keys((size_t)n, std::vector<cv::KeyPoint>(3));   // what the call must replace
  std::vector<cv::Mat> desc((size_t)n, cv::Mat(2, 32));
  std::vector<cv::Mat> grays(1, cv::Mat(2, 2));
  std::vector<int> mono;
  const auto t0 = std::chrono::steady_clock::now();
  ORBextractor::ExtractBatchRaw(extractors, images, prep, keys, desc, lapping, mono, keep_pyramid != 0, gray ? &grays : nullptr);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if ((int)keys.size() != n || (int)desc.size() != n || (int)mono.size() != n || (gray && (int)grays.size() != n)) return -1;
  for (int i = 0; i < n; ++i) {
    const osh_host_extract_output& o = out[i];
    if (o.call_ms) *o.call_ms = ms;
    *o.ret = mono[i]; *o.desc_rows = desc[i].rows;
    tokens[i] = extractors[i]->mnPyramidToken;
    PutPyramid(*extractors[i], in[i].nlevels, o);
    if (gray) {
      const cv::Mat& g = grays[i];
      gray_rows[i] = g.rows; gray_cols[i] = g.cols;
      if (gray[i] && (size_t)g.rows * g.cols <= (size_t)gray_capacity[i])
        for (int r = 0; r < g.rows; ++r) std::memcpy(gray[i] + (size_t)r * g.cols, g.ptr<uint8_t>(r), (size_t)g.cols);
    }
    if (mono[i] < 0) continue;   // an empty image: the extractor's outputs were not touched
    if (!PutKeypoints(keys[i], desc[i], o)) return -1;
  }
  return 0;
}

extern "C" int osh_host_frame_extract_and_match_stereo(const osh_host_extract_input* in, const osh_host_raw_image* raw, float bf, float b, int32_t chain,
                                                       const osh_host_extract_output* out, uint64_t* tokens, int32_t u_capacity, float* u_right, float* depth,
                                                       int32_t* n, uint8_t* const* gray, const int32_t* gray_capacity, int32_t* gray_rows, int32_t* gray_cols,
                                                       double* call_ms) {
  if (!in || !out || !tokens || !n || u_capacity < 0 || (u_capacity && (!u_right || !depth)) || (gray && (!raw || !gray_capacity || !gray_rows || !gray_cols))) return -1;
  std::vector<Standin> standins;
  standins.reserve(2);   // the extractors stay where they are
  std::vector<cv::Mat> images;
  std::vector<std::unique_ptr<RectifyMap> > maps;
  std::vector<ImagePrep> prep;
  for (int i = 0; i < 2; ++i) {
    const osh_host_extract_output& o = out[i];
    if (in[i].nlevels < 1 || in[i].rows < 0 || in[i].cols < 0 || (!raw && in[i].rows && in[i].cols && !in[i].pixels) || !o.level_rows || !o.level_cols || !o.ret ||
        !o.desc_rows || !o.pixels_needed || o.capacity < 0 || o.pixel_capacity < 0) return -1;
    osh_host_extract_input extractor = in[i];
    if (raw) extractor.rows = extractor.cols = 0;   // the stand-in's own image stays empty
    standins.emplace_back(extractor);
    if (!raw) { images.push_back(standins.back().image); continue; }
    const osh_host_raw_image& a = raw[i];
    if (a.rows < 0 || a.cols < 0 || a.channels < 1 || (a.rows && a.cols && !a.pixels) || (a.map_x && (!a.map_y || a.map_rows <= 0 || a.map_cols <= 0))) return -1;
    cv::Mat image;
    if (a.rows && a.cols) {
      image = cv::Mat(a.rows, a.cols, a.channels);
      std::memcpy(image.ptr<uint8_t>(0), a.pixels, (size_t)a.rows * a.cols * a.channels);
    }
    images.push_back(image);
    ImagePrep p;
    p.bRGB = a.rgb != 0; p.newRows = a.new_rows; p.newCols = a.new_cols;
    if (a.map_x) {
      const size_t step = sizeof(float) * (size_t)a.map_cols;
      maps.emplace_back(new RectifyMap(a.map_x, step, a.map_y, step, a.map_rows, a.map_cols, a.rows, a.cols));
      p.pMap = maps.back().get();
    }
    prep.push_back(p);
  }
  Frame F;
  F.mpORBextractorLeft = &standins[0].ex; F.mpORBextractorRight = &standins[1].ex;
  F.mbf = bf; F.mb = b;
  F.mvScaleFactors = standins[0].ex.mvScaleFactor; F.mvInvScaleFactors = standins[0].ex.mvInvScaleFactor;
  F.mvKeys.resize(3); F.mvKeysRight.resize(3); F.mvuRight.assign(3, 7.f); F.mvDepth.assign(3, 7.f); F.N = 3;   // what the call must replace
  std::vector<cv::Mat> grays(1, cv::Mat(2, 2));
  const auto t0 = std::chrono::steady_clock::now();
  if (chain) {   // the two calls the member replaces
    const std::vector<ORBextractor*> extractors{F.mpORBextractorLeft, F.mpORBextractorRight};
    const std::vector<std::vector<int> > lapping(2, std::vector<int>{0, 0});
    std::vector<std::vector<cv::KeyPoint> > keys;
    std::vector<cv::Mat> desc;
    std::vector<int> mono;
    if (raw) ORBextractor::ExtractBatchRaw(extractors, images, prep, keys, desc, lapping, mono, true, gray ? &grays : nullptr);
    else ORBextractor::ExtractBatch(extractors, images, keys, desc, lapping, mono, true);
    if (keys.size() != 2 || desc.size() != 2) return -1;
    F.mvKeys.swap(keys[0]); F.mvKeysRight.swap(keys[1]); F.mDescriptors = desc[0]; F.mDescriptorsRight = desc[1];   // as the member does
    F.N = (int)F.mvKeys.size();
    F.ComputeStereoMatches();
  } else {
    F.ExtractAndMatchStereo(images[0], images[1], raw ? &prep[0] : nullptr, raw ? &prep[1] : nullptr, gray ? &grays : nullptr);
  }
  if (call_ms) *call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  n[0] = F.N; n[1] = (int32_t)F.mvuRight.size(); n[2] = (int32_t)F.mvDepth.size(); n[3] = (int32_t)F.mvKeysRight.size();
  if (F.mvuRight.size() <= (size_t)u_capacity && F.mvDepth.size() <= (size_t)u_capacity) {
    if (!F.mvuRight.empty()) std::memcpy(u_right, F.mvuRight.data(), sizeof(float) * F.mvuRight.size());
    if (!F.mvDepth.empty()) std::memcpy(depth, F.mvDepth.data(), sizeof(float) * F.mvDepth.size());
  }
  const std::vector<cv::KeyPoint>* keys[2] = {&F.mvKeys, &F.mvKeysRight};
  const cv::Mat* desc[2] = {&F.mDescriptors, &F.mDescriptorsRight};
  for (int i = 0; i < 2; ++i) {
    const osh_host_extract_output& o = out[i];
    *o.ret = 0; *o.desc_rows = desc[i]->rows;
    tokens[i] = standins[i].ex.mnPyramidToken;
    PutPyramid(standins[i].ex, in[i].nlevels, o);
    if (gray) {
      const cv::Mat g = (size_t)i < grays.size() ? grays[i] : cv::Mat();
      gray_rows[i] = g.rows; gray_cols[i] = g.cols;
      if (gray[i] && (size_t)g.rows * g.cols <= (size_t)gray_capacity[i])
        for (int r = 0; r < g.rows; ++r) std::memcpy(gray[i] + (size_t)r * g.cols, g.ptr<uint8_t>(r), (size_t)g.cols);
    }
    if (!PutKeypoints(*keys[i], *desc[i], o)) return -1;
  }
  return 0;
}

extern "C" int osh_host_orb_prepare_cpu(int32_t n_frames, const osh_prepare_frame* frames, const osh_rectify_map_desc* const* maps,
                                        osh_prepare_result* results, double* ms) {
  if (n_frames < 0 || (n_frames && (!frames || !results))) return -1;
  // the checks of osh_rectify_map_create and osh_orb_prepare, in their order
  for (int k = 0; k < n_frames; ++k) {
    const osh_prepare_frame& f = frames[k];
    const osh_prepare_image& im = f.image;
    const osh_rectify_map_desc* m = maps ? maps[k] : nullptr;
    if (f.map || !results[k].gray) return -1;
    if (m) {
      if (!m->map_x || !m->map_y || m->rows <= 0 || m->cols <= 0 || m->src_rows <= 0 || m->src_cols <= 0) return OSH_ERR_INVALID;
      if (m->map_x_stride < 4 * (int64_t)m->cols || m->map_y_stride < 4 * (int64_t)m->cols) return OSH_ERR_INVALID;
      if (m->rows > OSH_FAST_MAX_SIDE || m->cols > OSH_FAST_MAX_SIDE || m->src_rows > OSH_FAST_MAX_SIDE || m->src_cols > OSH_FAST_MAX_SIDE) return OSH_ERR_UNSUPPORTED;
    }
    if (!im.data || im.rows <= 0 || im.cols <= 0) return OSH_ERR_INVALID;
    if (im.channels != 1 && im.channels != 3 && im.channels != 4) return OSH_ERR_INVALID;
    if (im.stride < (int64_t)im.cols * im.channels) return OSH_ERR_INVALID;
    if (f.order != OSH_PREP_RGB && f.order != OSH_PREP_BGR) return OSH_ERR_INVALID;
    if (m && (m->src_rows != im.rows || m->src_cols != im.cols)) return OSH_ERR_INVALID;
    int rows = f.out_rows, cols = f.out_cols;
    if (rows == 0 && cols == 0) { rows = m ? m->rows : im.rows; cols = m ? m->cols : im.cols; }
    if (rows <= 0 || cols <= 0) return OSH_ERR_INVALID;
    if (m && (rows != m->rows || cols != m->cols)) return OSH_ERR_INVALID;
    if (results[k].gray_stride < (int64_t)cols) return OSH_ERR_INVALID;
    if (im.rows > OSH_FAST_MAX_SIDE || im.cols > OSH_FAST_MAX_SIDE || rows > OSH_FAST_MAX_SIDE || cols > OSH_FAST_MAX_SIDE) return OSH_ERR_UNSUPPORTED;
    results[k].rows = rows; results[k].cols = cols;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_frames; ++k) {
    const osh_prepare_frame& f = frames[k];
    const osh_rectify_map_desc* m = maps ? maps[k] : nullptr;
    const osh::PrepSource S{f.image.data, (long long)f.image.stride, f.image.rows, f.image.cols, f.image.channels, f.order == OSH_PREP_BGR ? osh::kPrepBGR : osh::kPrepRGB};
    osh::prep_frame_host(S, m ? m->map_x : nullptr, m ? (long long)m->map_x_stride : 0, m ? m->map_y : nullptr, m ? (long long)m->map_y_stride : 0,
                         results[k].gray, results[k].rows, results[k].cols, (long long)results[k].gray_stride);
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}
