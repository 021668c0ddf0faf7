// orbextractor_io.h -- what the C wrappers around the stand-in ORB_SLAM3::ORBextractor share (csrc/hosttest/orbextractor.cc and
// csrc/hosttest/prepare.cc): a stand-in extractor with its image made from an osh_host_extract_input, and the writers of an
// osh_host_extract_output.  Test library only.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "ORBextractor.h"
#include "orb_extract_steps.h"
#include "orbslam3_hip_host.h"

namespace {

using ORB_SLAM3::ORBextractor;
using ORB_SLAM3::kEdge;

// The stand-in extractor, the image (empty: no rows or no columns) and the lapping area of an osh_host_extract_input
struct Standin {
  ORBextractor ex;
  cv::Mat image;
  std::vector<int> lapping;
  explicit Standin(const osh_host_extract_input& in)
      : ex(in.nfeatures, in.scale_factor, in.nlevels, in.ini_th, in.min_th), lapping{in.lapping[0], in.lapping[1]} {
    if (!in.rows || !in.cols) return;
    image = cv::Mat(in.rows, in.cols);
    std::memcpy(image.ptr<uint8_t>(0), in.pixels, (size_t)in.rows * in.cols);
  }
};

// The keypoints of `all`, level after level: the count of every level, and while there is room (`capacity`) the fields whose array
// is not null.  Returns how many keypoints there are, so a first pass without room counts
int PutLevelKeypoints(const std::vector<std::vector<cv::KeyPoint> >& all, int nlevels, int32_t capacity, int32_t* level_count, float* xy, float* angle,
                      float* response, float* size = nullptr, int32_t* octave = nullptr) {
  size_t n = 0;
  for (int l = 0; l < nlevels; ++l) {
    level_count[l] = (int32_t)all[l].size();
    for (const cv::KeyPoint& kp : all[l]) {
      if (n < (size_t)capacity) {
        if (xy) { xy[2 * n] = kp.pt.x; xy[2 * n + 1] = kp.pt.y; }
        if (angle) angle[n] = kp.angle;
        if (response) response[n] = kp.response;
        if (size) size[n] = kp.size;
        if (octave) octave[n] = kp.octave;
      }
      ++n;
    }
  }
  return (int)n;
}

// The shapes of the extractor's levels and, while they fit pixel_capacity, their pixels one after the other without the borders
void PutPyramid(const ORBextractor& ex, int nlevels, const osh_host_extract_output& o) {
  size_t pixels = 0;
  for (int l = 0; l < nlevels; ++l) {
    const cv::Mat im = l < (int)ex.mvImagePyramid.size() ? ex.mvImagePyramid[l] : cv::Mat();
    o.level_rows[l] = im.rows; o.level_cols[l] = im.cols;
    if (o.pyramid && pixels + (size_t)im.rows * im.cols <= (size_t)o.pixel_capacity)
      for (int r = 0; r < im.rows; ++r) std::memcpy(o.pyramid + pixels + (size_t)r * im.cols, im.ptr<uint8_t>(r), (size_t)im.cols);
    pixels += (size_t)im.rows * im.cols;
  }
  *o.pixels_needed = (int32_t)pixels;
}

// _keypoints and _descriptors as a call left them, the first `capacity` of them.  False: the descriptors are not [keys.size(), 32]
bool PutKeypoints(const std::vector<cv::KeyPoint>& keys, const cv::Mat& desc, const osh_host_extract_output& o) {
  if (!keys.empty() && (desc.rows != (int)keys.size() || desc.cols != 32)) return false;
  for (size_t i = 0; i < keys.size() && i < (size_t)o.capacity; ++i) {
    if (o.xy) { o.xy[2 * i] = keys[i].pt.x; o.xy[2 * i + 1] = keys[i].pt.y; }
    if (o.angle) o.angle[i] = keys[i].angle;
    if (o.size) o.size[i] = keys[i].size;
    if (o.response) o.response[i] = keys[i].response;
    if (o.octave) o.octave[i] = keys[i].octave;
    if (o.descriptors) std::memcpy(o.descriptors + 32 * i, desc.ptr<uint8_t>((int)i), 32);
  }
  return true;
}

// The whole bordered image of a level (the level is a view at (19, 19) of it) into `dst`, its rows im.step bytes apart there too
void CopyBordered(const cv::Mat& im, uint8_t* dst) {
  for (int r = -kEdge; r < im.rows + kEdge; ++r) std::memcpy(dst + (size_t)(r + kEdge) * im.step, im.ptr<uint8_t>(0) + (long long)r * (long long)im.step - kEdge, im.step);
}

}  // namespace
