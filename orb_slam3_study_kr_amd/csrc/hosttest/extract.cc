// extract.cc -- the C wrapper that drives ORBextractor::ExtractBatch (csrc/host/ORBextractor.cc) on stand-in extractors:
// osh_host_orbextractor_extract_batch (include/orbslam3_hip_host.h).  Test library only.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "ORBextractor.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

extern "C" int osh_host_orbextractor_extract_batch(int32_t n, const osh_host_extract_input* in, const osh_host_extract_output* out, int32_t keep_pyramid,
                                                   uint64_t* tokens) {
  if (n < 0 || (n && (!in || !out || !tokens))) return -1;
  std::vector<std::unique_ptr<ORB_SLAM3::ORBextractor> > owned;
  std::vector<ORB_SLAM3::ORBextractor*> extractors;
  std::vector<cv::Mat> images((size_t)n);
  std::vector<std::vector<int> > lapping;
  for (int i = 0; i < n; ++i) {
    const osh_host_extract_input& a = in[i];
    const osh_host_extract_output& o = out[i];
    if (a.nlevels < 1 || a.rows < 0 || a.cols < 0 || (a.rows && a.cols && !a.pixels) || !o.level_rows || !o.level_cols || !o.ret || !o.desc_rows || !o.pixels_needed ||
        o.capacity < 0 || o.pixel_capacity < 0) return -1;
    owned.emplace_back(new ORB_SLAM3::ORBextractor(a.nfeatures, a.scale_factor, a.nlevels, a.ini_th, a.min_th));
    extractors.push_back(owned.back().get());
    if (a.rows && a.cols) {
      images[i] = cv::Mat(a.rows, a.cols);
      std::memcpy(images[i].ptr<uint8_t>(0), a.pixels, (size_t)a.rows * a.cols);
    }
    lapping.push_back({a.lapping[0], a.lapping[1]});
  }
  std::vector<std::vector<cv::KeyPoint> > keys((size_t)n, std::vector<cv::KeyPoint>(3));   // what the call must replace
  std::vector<cv::Mat> desc((size_t)n, cv::Mat(2, 32));
  std::vector<int> mono;
  const auto t0 = std::chrono::steady_clock::now();
  ORB_SLAM3::ORBextractor::ExtractBatch(extractors, images, keys, desc, lapping, mono, keep_pyramid != 0);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if ((int)keys.size() != n || (int)desc.size() != n || (int)mono.size() != n) return -1;
  for (int i = 0; i < n; ++i) {
    const osh_host_extract_output& o = out[i];
    const ORB_SLAM3::ORBextractor& ex = *extractors[i];
    if (o.call_ms) *o.call_ms = ms;
    *o.ret = mono[i]; *o.desc_rows = desc[i].rows;
    tokens[i] = ex.mnPyramidToken;
    size_t pixels = 0;
    for (int l = 0; l < in[i].nlevels; ++l) {
      const cv::Mat im = l < (int)ex.mvImagePyramid.size() ? ex.mvImagePyramid[l] : cv::Mat();
      o.level_rows[l] = im.rows; o.level_cols[l] = im.cols;
      if (o.pyramid && pixels + (size_t)im.rows * im.cols <= (size_t)o.pixel_capacity)
        for (int r = 0; r < im.rows; ++r) std::memcpy(o.pyramid + pixels + (size_t)r * im.cols, im.ptr<uint8_t>(r), (size_t)im.cols);
      pixels += (size_t)im.rows * im.cols;
    }
    *o.pixels_needed = (int32_t)pixels;
    if (mono[i] < 0) continue;   // an empty image: the extractor's outputs were not touched
    if (!keys[i].empty() && (desc[i].rows != (int)keys[i].size() || desc[i].cols != 32)) return -1;
    for (size_t k = 0; k < keys[i].size() && k < (size_t)o.capacity; ++k) {
      if (o.xy) { o.xy[2 * k] = keys[i][k].pt.x; o.xy[2 * k + 1] = keys[i][k].pt.y; }
      if (o.angle) o.angle[k] = keys[i][k].angle;
      if (o.size) o.size[k] = keys[i][k].size;
      if (o.response) o.response[k] = keys[i][k].response;
      if (o.octave) o.octave[k] = keys[i][k].octave;
      if (o.descriptors) std::memcpy(o.descriptors + 32 * k, desc[i].ptr<uint8_t>((int)k), 32);
    }
  }
  return 0;
}
