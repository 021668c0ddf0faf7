// orbextractor.cc -- what the stand-in ORB_SLAM3::ORBextractor (include/ORBextractor.h) needs around
// ORBextractor::ComputeKeyPointsOctTree and ORBextractor::operator() (csrc/host/ORBextractor.cc), and the C wrappers that drive them
// (include/orbslam3_hip_host.h): the constructor (scale tables and mnFeaturesPerLevel as reference src/ORBextractor.cc:409-447, and
// a generated sampling table), a DistributeOctTree test double, osh_host_orbextractor_compute_keypoints,
// osh_host_orbextractor_extract, osh_host_orbextractor_extract_batch, osh_host_orbextractor_compute_pyramid, and csrc/orb_fast.h / csrc/orb_brief.h / csrc/orb_pyramid.h
// on the host in one thread (osh_host_orb_fast_cpu, osh_host_orb_ic_angle_cpu, osh_host_orb_describe_cpu, osh_host_orb_pyramid_cpu:
// the CPU baselines of profiles/fast_timing.py, profiles/brief_timing.py and profiles/pyramid_timing.py;
// osh_host_orb_fast_level_cells).  Test library only.  ComputePyramid is the product body of csrc/host/ORBextractor.cc.
//
// The sampling table is this file's own: 512 points drawn by a fixed linear congruential generator, uniformly in [-13, 12]^2 (so
// the radius is at most sqrt(338) = 18.38), the first one set to (-13, -13) so that the reach is 19 as for the reference's table.
//
// The DistributeOctTree here is written from the behaviour, not taken from the reference: a quadtree over the level's detect area
// that splits the nodes holding more than one keypoint until there are nFeatures nodes (or nothing left to split), the fullest
// nodes first once a whole round would overshoot, and keeps the strongest keypoint of every node.  The reference sorts
// pair<int, ExtractorNode*> and so breaks ties between equally full nodes by pointer value; this double breaks them by the order in
// which the nodes were created.  Its selection is therefore its own and no test compares it with anything else.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ORBextractor.h"
#include "orb_extract_steps.h"
#include "orbextractor_io.h"
#include "../orb_brief.h"
#include "../orb_fast.h"
#include "../orb_pyramid.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

namespace ORB_SLAM3 {

ORBextractor::ORBextractor(int _nfeatures, float _scaleFactor, int _nlevels, int _iniThFAST, int _minThFAST)
    : nfeatures(_nfeatures), scaleFactor(_scaleFactor), nlevels(_nlevels), iniThFAST(_iniThFAST), minThFAST(_minThFAST) {
  mvScaleFactor.resize(nlevels); mvLevelSigma2.resize(nlevels);
  mvInvScaleFactor.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
  for (int i = 0; i < nlevels; i++) {
    mvScaleFactor[i] = i ? (float)(mvScaleFactor[i - 1] * scaleFactor) : 1.0f;
    mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i];
    mvInvScaleFactor[i] = 1.0f / mvScaleFactor[i];
    mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i];
  }
  mvImagePyramid.resize(nlevels);
  // the features of a level: a geometric series over the levels that sums to nfeatures, each term rounded half to even, the last
  // level taking what is left
  mnFeaturesPerLevel.assign(nlevels, 0);
  const float q = 1.0f / scaleFactor;                                                         // ratio of the series
  float share = nfeatures * (1 - q) / (1 - (float)std::pow((double)q, (double)nlevels));      // of level 0, in float32 steps
  int given = 0;
  for (int l = 0; l + 1 < nlevels; ++l, share *= q) given += mnFeaturesPerLevel[l] = (int)std::nearbyint(share);
  if (nlevels > 0) mnFeaturesPerLevel[nlevels - 1] = std::max(nfeatures - given, 0);
  pattern.resize(512);
  uint32_t state = 0x0b5e55edu;
  for (cv::Point& p : pattern) {
    state = state * 1664525u + 1013904223u; p.x = (int)((state >> 8) % 26u) - 13;
    state = state * 1664525u + 1013904223u; p.y = (int)((state >> 8) % 26u) - 13;
  }
  pattern[0] = cv::Point(-13, -13);
}

namespace {
struct OctNode {
  int x0, x1, y0, y1;        // [x0, x1) x [y0, y1), relative to (minX, minY) like the keypoints
  std::vector<int> keys;     // indices into vToDistributeKeys, ascending
  bool splittable() const { return keys.size() > 1 && (x1 - x0 > 1 || y1 - y0 > 1); }
};
}  // namespace

std::vector<cv::KeyPoint> ORBextractor::DistributeOctTree(const std::vector<cv::KeyPoint>& vToDistributeKeys, const int& minX, const int& maxX,
                                                          const int& minY, const int& maxY, const int& N, const int& level) {
  mvDistributeCalls.push_back({vToDistributeKeys, minX, maxX, minY, maxY, N, level});
  std::vector<cv::KeyPoint> result;
  const int W = maxX - minX, H = maxY - minY;
  if (vToDistributeKeys.empty() || W <= 0 || H <= 0) return result;
  // roots: as many side by side as the area is wider than high
  const int nIni = std::max(1, (int)std::nearbyint((float)W / (float)H));
  std::vector<OctNode> nodes(nIni);   // in creation order
  for (int r = 0; r < nIni; ++r) nodes[r] = {(int)((long long)W * r / nIni), (int)((long long)W * (r + 1) / nIni), 0, H, {}};
  for (int k = 0; k < (int)vToDistributeKeys.size(); ++k) {
    int r = 0;
    while (r + 1 < nIni && vToDistributeKeys[k].pt.x >= (float)nodes[r].x1) ++r;
    nodes[r].keys.push_back(k);
  }
  nodes.erase(std::remove_if(nodes.begin(), nodes.end(), [](const OctNode& n) { return n.keys.empty(); }), nodes.end());

  auto split = [&](size_t at) {   // the node at `at` leaves, its non-empty quarters join at the end
    const OctNode n = nodes[at];
    nodes.erase(nodes.begin() + (long)at);
    const int mx = n.x0 + (n.x1 - n.x0 + 1) / 2, my = n.y0 + (n.y1 - n.y0 + 1) / 2;
    OctNode q[4] = {{n.x0, mx, n.y0, my, {}}, {mx, n.x1, n.y0, my, {}}, {n.x0, mx, my, n.y1, {}}, {mx, n.x1, my, n.y1, {}}};
    for (int k : n.keys) q[(vToDistributeKeys[k].pt.x >= (float)mx ? 1 : 0) + (vToDistributeKeys[k].pt.y >= (float)my ? 2 : 0)].keys.push_back(k);
    for (const OctNode& c : q) if (!c.keys.empty()) nodes.push_back(c);
  };
  while ((int)nodes.size() < N) {
    std::vector<size_t> open;
    for (size_t k = 0; k < nodes.size(); ++k) if (nodes[k].splittable()) open.push_back(k);
    if (open.empty()) break;
    const size_t before = nodes.size();
    if ((int)(nodes.size() + 3 * open.size()) > N) {
      // a whole round would overshoot: the fullest node first, one at a time (ties: the node created first)
      size_t best = open[0];
      for (size_t k : open) if (nodes[k].keys.size() > nodes[best].keys.size()) best = k;
      split(best);
    } else {
      for (size_t k = open.size(); k-- > 0;) split(open[k]);   // back to front: the indices in front stay valid
    }
    if (nodes.size() == before) {
      bool shrunk = false;   // no node more, but the boxes got smaller: go on until they cannot
      for (const OctNode& n : nodes) shrunk |= n.splittable();
      if (!shrunk) break;
    }
  }
  result.reserve(nodes.size());
  for (const OctNode& n : nodes) {
    int best = n.keys[0];
    for (int k : n.keys) if (vToDistributeKeys[k].response > vToDistributeKeys[best].response) best = k;
    result.push_back(vToDistributeKeys[best]);
  }
  return result;
}

}  // namespace ORB_SLAM3

using namespace ORB_SLAM3;

extern "C" int osh_host_orb_fast_cpu(int32_t n_frames, const osh_fast_frame* frames, osh_fast_result* results, double* ms) {
  if (n_frames < 0 || (n_frames && (!frames || !results))) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_frames; ++k) {
    const osh_fast_frame& f = frames[k];
    osh_fast_result& r = results[k];
    if (!f.pyramid || !r.level_count) return -1;
    std::vector<osh::FastCorner> corners;
    std::vector<uint8_t> used;
    std::vector<int> level_of;
    for (int l = 0; l < f.n_levels; ++l) {
      const size_t before = corners.size();
      osh::fast_level_host(f.pyramid[l].data, f.pyramid[l].rows, f.pyramid[l].cols, (long long)f.pyramid[l].stride, f.ini_th, f.min_th, 0, corners, used);
      r.level_count[l] = (int32_t)(corners.size() - before);
      level_of.resize(corners.size(), l);
    }
    r.n_out = (int32_t)corners.size(); r.n_cells = (int32_t)used.size(); r.pyramid_token = 0;
    if (r.n_out > r.capacity || (r.used_min_th && r.n_cells > r.cell_capacity)) continue;
    if (r.used_min_th) std::copy(used.begin(), used.end(), r.used_min_th);
    for (size_t i = 0; i < corners.size(); ++i) {
      r.xy[2 * i] = corners[i].x; r.xy[2 * i + 1] = corners[i].y; r.response[i] = corners[i].response;
      if (r.level) r.level[i] = level_of[i];
      if (r.cell) r.cell[i] = corners[i].cell;
    }
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_orb_ic_angle_cpu(int32_t n_frames, const osh_ic_angle_frame* frames, const osh_ic_angle_result* results, double* ms) {
  if (n_frames < 0 || (n_frames && (!frames || !results))) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_frames; ++k) {
    const osh_ic_angle_frame& f = frames[k];
    if (!f.pyramid || (f.n && (!f.xy || !f.level))) return -1;
    for (int i = 0; i < f.n; ++i) {
      const osh_stereo_image& im = f.pyramid[f.level[i]];
      int m10, m01;
      const float a = osh::fast_ic_angle_host(im.data, (long long)im.stride, f.xy[2 * i], f.xy[2 * i + 1], m10, m01);
      if (results[k].angle) results[k].angle[i] = a;
      if (results[k].m10) results[k].m10[i] = m10;
      if (results[k].m01) results[k].m01[i] = m01;
    }
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_orb_pyramid_cpu(int32_t n_frames, const osh_pyramid_frame* frames, osh_pyramid_result* results, double* ms) {
  if (n_frames < 0 || (n_frames && (!frames || !results))) return -1;
  // the checks of osh_orb_pyramid_build, in its order
  std::vector<std::vector<int> > rows(n_frames), cols(n_frames);
  for (int k = 0; k < n_frames; ++k) {
    const osh_pyramid_frame& f = frames[k];
    const osh_pyramid_result& r = results[k];
    if (!f.image.data || f.image.rows <= 0 || f.image.cols <= 0 || f.image.stride < f.image.cols) return OSH_ERR_INVALID;
    if (f.image.rows > OSH_FAST_MAX_SIDE || f.image.cols > OSH_FAST_MAX_SIDE) return OSH_ERR_UNSUPPORTED;
    if (f.n_levels < 1 || f.n_levels > OSH_STEREO_MAX_LEVELS || !f.inv_scale || r.border < 0) return OSH_ERR_INVALID;
    for (int l = 0; l < f.n_levels; ++l) {
      const float inv = f.inv_scale[l];
      if (!std::isfinite(inv) || !(inv > 0.f)) return OSH_ERR_INVALID;
      const int h = osh::pyr_level_size(f.image.rows, inv), w = osh::pyr_level_size(f.image.cols, inv);
      if (h <= 0 || w <= 0) return OSH_ERR_INVALID;
      if (l == 0 && (h != f.image.rows || w != f.image.cols)) return OSH_ERR_INVALID;
      if (h > OSH_FAST_MAX_SIDE || w > OSH_FAST_MAX_SIDE) return OSH_ERR_UNSUPPORTED;
      if (r.levels && (!r.levels[l].data || r.levels[l].rows != h || r.levels[l].cols != w || r.levels[l].stride < (int64_t)w + 2 * (int64_t)r.border)) return OSH_ERR_INVALID;
      rows[k].push_back(h); cols[k].push_back(w);
    }
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_frames; ++k) {
    const osh_pyramid_frame& f = frames[k];
    osh_pyramid_result& r = results[k];
    std::vector<std::vector<uint8_t> > own(f.n_levels);   // the levels nobody asked for
    const uint8_t* prev = nullptr;
    long long prev_stride = 0;
    for (int l = 0; l < f.n_levels; ++l) {
      const int h = rows[k][l], w = cols[k][l];
      uint8_t* dst;
      long long stride;
      if (r.levels) { dst = r.levels[l].data; stride = (long long)r.levels[l].stride; }
      else { own[l].resize((size_t)h * w); dst = own[l].data(); stride = w; }
      if (l == 0) for (int y = 0; y < h; ++y) std::memcpy(dst + y * stride, f.image.data + y * (long long)f.image.stride, (size_t)w);
      else osh::pyr_resample_level_host(prev, rows[k][l - 1], cols[k][l - 1], prev_stride, dst, h, w, stride);
      if (r.levels) osh::pyr_border_host(dst, h, w, stride, r.border);
      if (r.level_rows) r.level_rows[l] = h;
      if (r.level_cols) r.level_cols[l] = w;
      prev = dst; prev_stride = stride;
    }
    r.pyramid_token = 0;
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_orbextractor_compute_pyramid(const osh_host_extract_input* in, const osh_host_pyramid_output* out) {
  if (!in || !out || in->nlevels < 1 || in->rows <= 0 || in->cols <= 0 || !in->pixels || !out->level_rows || !out->level_cols || !out->pixels_needed ||
      !out->level_count || !out->hand_level_count || !out->built_token || out->capacity < 0 || out->pixel_capacity < 0) return -1;
  Standin s(*in);
  ORBextractor& ex = s.ex;
  ex.ComputePyramid(s.image);
  out->built_token[0] = ex.mnBuiltPyramidToken; out->built_token[1] = 0;
  if ((int)ex.mvImagePyramid.size() != in->nlevels) return -2;
  // the whole bordered images: the levels are views at (19, 19) of them
  size_t pixels = 0;
  for (int l = 0; l < in->nlevels; ++l) {
    const cv::Mat& im = ex.mvImagePyramid[l];
    out->level_rows[l] = im.rows; out->level_cols[l] = im.cols;
    if (im.empty()) continue;
    if (im.step != (size_t)im.cols + 2 * kEdge) return -2;
    const size_t bytes = (size_t)(im.rows + 2 * kEdge) * im.step;
    if (out->bordered && pixels + bytes <= (size_t)out->pixel_capacity) CopyBordered(im, out->bordered + pixels);
    pixels += bytes;
  }
  *out->pixels_needed = (int32_t)pixels;
  // ComputeKeyPointsOctTree right after ComputePyramid (the resident levels), then on a hand-set copy of that pyramid
  std::vector<std::vector<cv::KeyPoint> > all;
  ex.ComputeKeyPointsOctTree(all);
  if ((int)all.size() != in->nlevels) return -2;
  const int n = PutLevelKeypoints(all, in->nlevels, out->capacity, out->level_count, out->xy, out->angle, out->response);
  for (int l = 0; l < in->nlevels; ++l) {
    const cv::Mat im = ex.mvImagePyramid[l];
    if (im.empty()) continue;
    cv::Mat whole(im.rows + 2 * kEdge, im.cols + 2 * kEdge);
    CopyBordered(im, whole.ptr<uint8_t>(0));
    ex.mvImagePyramid[l] = whole.view(kEdge, kEdge, im.rows, im.cols);
  }
  out->built_token[1] = ex.mnBuiltPyramidToken;   // 0: the first call consumed it
  ex.ComputeKeyPointsOctTree(all);
  if ((int)all.size() != in->nlevels) return -2;
  const int n_hand = PutLevelKeypoints(all, in->nlevels, out->capacity, out->hand_level_count, out->hand_xy, out->hand_angle, out->hand_response);
  return std::max(n, n_hand);
}

extern "C" int osh_host_orb_fast_level_cells(int32_t rows, int32_t cols, int32_t geom[6], int32_t* rects) {
  if (rows <= 0 || cols <= 0 || !geom) return -1;
  const osh::FastGeom g = osh::fast_geometry(rows, cols);
  geom[0] = g.n_cols; geom[1] = g.n_rows; geom[2] = g.w_cell; geom[3] = g.h_cell; geom[4] = g.max_x; geom[5] = g.max_y;
  int n = 0;
  osh::FastRect r;
  for (int i = 0; i < g.n_rows; ++i)
    for (int j = 0; j < g.n_cols; ++j) {
      if (!osh::fast_cell_rect(g, i, j, r)) continue;
      if (rects) { rects[4 * n] = r.x0; rects[4 * n + 1] = r.y0; rects[4 * n + 2] = r.w; rects[4 * n + 3] = r.h; }
      ++n;
    }
  return n;
}

extern "C" int osh_host_orbextractor_compute_keypoints(const osh_host_orbextractor_input* in, const osh_host_orbextractor_output* out) {
  if (!in || !out || in->nlevels < 0 || in->n_images < 0 || in->border < 0 || (in->n_images && (!in->rows || !in->cols || !in->pixels)) || !out->level_count ||
      !out->cand_level_count) return -1;
  ORBextractor ex(in->nfeatures, in->scale_factor, in->nlevels, in->ini_th, in->min_th);
  // levels as views into bordered images, like the reference's ComputePyramid leaves them
  ex.mvImagePyramid.resize(in->n_images);
  size_t off = 0;
  for (int l = 0; l < in->n_images; ++l) {
    cv::Mat whole(in->rows[l] + 2 * in->border, in->cols[l] + 2 * in->border);
    for (int r = 0; r < whole.rows; ++r) std::memset(whole.ptr<uint8_t>(r), 167, (size_t)whole.cols);
    ex.mvImagePyramid[l] = whole.view(in->border, in->border, in->rows[l], in->cols[l]);
    for (int r = 0; r < in->rows[l]; ++r) std::memcpy(ex.mvImagePyramid[l].ptr<uint8_t>(r), in->pixels + off + (size_t)r * in->cols[l], (size_t)in->cols[l]);
    off += (size_t)in->rows[l] * in->cols[l];
  }
  std::vector<std::vector<cv::KeyPoint> > all;
  ex.ComputeKeyPointsOctTree(all);
  if ((int)all.size() != in->nlevels) return -2;
  for (int l = 0; l < in->nlevels; ++l) {
    out->cand_level_count[l] = 0;
    if (out->features_per_level) out->features_per_level[l] = ex.mnFeaturesPerLevel[l];
    if (out->scale_factors) out->scale_factors[l] = ex.mvScaleFactor[l];
  }
  size_t nc = 0;
  for (const ORBextractor::DistributeCall& d : ex.mvDistributeCalls) {
    if (d.level < 0 || d.level >= in->nlevels) return -2;
    out->cand_level_count[d.level] += (int32_t)d.keys.size();
    if (out->cand_args) { int32_t* a = out->cand_args + 6 * d.level; a[0] = d.minX; a[1] = d.maxX; a[2] = d.minY; a[3] = d.maxY; a[4] = d.nFeatures; a[5] = d.level; }
    for (const cv::KeyPoint& kp : d.keys) {
      if (nc < (size_t)out->cand_capacity) {
        if (out->cand_xy) { out->cand_xy[2 * nc] = kp.pt.x; out->cand_xy[2 * nc + 1] = kp.pt.y; }
        if (out->cand_response) out->cand_response[nc] = kp.response;
      }
      ++nc;
    }
  }
  return PutLevelKeypoints(all, in->nlevels, out->capacity, out->level_count, out->xy, out->angle, out->response, out->size, out->octave);
}

extern "C" int osh_host_orb_describe_cpu(int32_t n_frames, const osh_describe_frame* frames, const osh_describe_result* results, double* ms) {
  if (n_frames < 0 || (n_frames && (!frames || !results))) return -1;
  uint16_t default_w[osh::kBriefTaps];
  osh::brief_gaussian_q8(osh::kBriefTaps, 2.0, default_w);
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n_frames; ++k) {
    const osh_describe_frame& f = frames[k];
    const osh_describe_result& r = results[k];
    if (!f.pyramid || !f.pattern || (f.n && (!f.xy || !f.level || !f.angle || !r.descriptors))) return -1;
    const uint16_t* w = f.blur_q8 ? f.blur_q8 : default_w;
    std::vector<std::vector<uint8_t> > blurred(f.n_levels);
    std::vector<bool> wanted(f.n_levels, r.blurred != nullptr);
    for (int i = 0; i < f.n; ++i) wanted[f.level[i]] = true;
    size_t off = 0;
    for (int l = 0; l < f.n_levels; ++l) {
      const osh_stereo_image& im = f.pyramid[l];
      const size_t bytes = (size_t)im.rows * im.cols;
      if (wanted[l]) {
        if (im.rows < osh::kBriefMinSide || im.cols < osh::kBriefMinSide) return -1;
        blurred[l].resize(bytes);
        osh::brief_blur_level_host(im.data, im.rows, im.cols, (long long)im.stride, w, blurred[l].data());
        if (r.blurred) std::memcpy(r.blurred + off, blurred[l].data(), bytes);
      }
      off += bytes;
    }
    for (int i = 0; i < f.n; ++i) {
      const int l = f.level[i];
      const osh::BriefRot rot = osh::brief_descriptor_host(blurred[l].data(), (long long)f.pyramid[l].cols, f.xy[2 * i], f.xy[2 * i + 1], f.angle[i], f.pattern,
                                                           r.descriptors + 32 * (size_t)i);
      if (r.cos_sin) { r.cos_sin[2 * i] = rot.a; r.cos_sin[2 * i + 1] = rot.b; }
    }
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int osh_host_brief_gaussian_q8(int32_t ksize, double sigma, uint16_t* out) {
  if (ksize < 1 || ksize > 31 || !(ksize & 1) || !(sigma > 0) || !out) return -1;
  osh::brief_gaussian_q8(ksize, sigma, out);
  return 0;
}

extern "C" int osh_host_brief_reach(const int8_t* pattern) { return pattern ? osh::brief_reach(pattern) : -1; }

extern "C" int osh_host_orbextractor_pattern(int8_t* pattern) {
  if (!pattern) return -1;
  PatternTable(ORBextractor(1, 1.2f, 1, 20, 7).pattern.data(), pattern);
  return 0;
}

extern "C" int osh_host_orbextractor_extract(const osh_host_extract_input* in, const osh_host_extract_output* out) {
  if (!in || !out || in->nlevels < 1 || in->rows < 0 || in->cols < 0 || (in->rows && in->cols && !in->pixels) || !out->level_rows || !out->level_cols ||
      !out->level_count || !out->ret || !out->desc_rows || !out->pixels_needed || out->capacity < 0 || out->pixel_capacity < 0) return -1;
  Standin s(*in);
  ORBextractor& ex = s.ex;
  // the stages on their own first: what operator() computes inside is a function of the image alone
  std::vector<std::vector<cv::KeyPoint> > all(in->nlevels);
  if (!s.image.empty()) {
    ex.ComputePyramid(s.image);
    ex.ComputeKeyPointsOctTree(all);
    if ((int)all.size() != in->nlevels) return -1;
  }
  PutPyramid(ex, in->nlevels, *out);
  PutLevelKeypoints(all, in->nlevels, out->capacity, out->level_count, out->level_xy, out->level_angle, nullptr);
  std::vector<cv::KeyPoint> keys(3);   // what the call must replace
  cv::Mat desc(2, 32);
  const auto t0 = std::chrono::steady_clock::now();
  *out->ret = ex(s.image, cv::Mat(), keys, desc, s.lapping);
  if (out->call_ms) *out->call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out->desc_rows = desc.rows;
  if (*out->ret < 0) return 0;   // an empty image: nothing was touched
  if (!PutKeypoints(keys, desc, *out)) return -1;
  return (int)keys.size();
}

extern "C" int osh_host_orbextractor_extract_batch(int32_t n, const osh_host_extract_input* in, const osh_host_extract_output* out, int32_t keep_pyramid,
                                                   uint64_t* tokens) {
  if (n < 0 || (n && (!in || !out || !tokens))) return -1;
  std::vector<Standin> standins;
  standins.reserve((size_t)(n > 0 ? n : 0));   // the extractors stay where they are
  for (int i = 0; i < n; ++i) {
    const osh_host_extract_input& a = in[i];
    const osh_host_extract_output& o = out[i];
    if (a.nlevels < 1 || a.rows < 0 || a.cols < 0 || (a.rows && a.cols && !a.pixels) || !o.level_rows || !o.level_cols || !o.ret || !o.desc_rows || !o.pixels_needed ||
        o.capacity < 0 || o.pixel_capacity < 0) return -1;
    standins.emplace_back(a);
  }
  std::vector<ORBextractor*> extractors;
  std::vector<cv::Mat> images;
  std::vector<std::vector<int> > lapping;
  for (Standin& s : standins) { extractors.push_back(&s.ex); images.push_back(s.image); lapping.push_back(s.lapping); }
  std::vector<std::vector<cv::KeyPoint> > keys((size_t)n, std::vector<cv::KeyPoint>(3));   // what the call must replace
  std::vector<cv::Mat> desc((size_t)n, cv::Mat(2, 32));
  std::vector<int> mono;
  const auto t0 = std::chrono::steady_clock::now();
  ORBextractor::ExtractBatch(extractors, images, keys, desc, lapping, mono, keep_pyramid != 0);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if ((int)keys.size() != n || (int)desc.size() != n || (int)mono.size() != n) return -1;
  for (int i = 0; i < n; ++i) {
    const osh_host_extract_output& o = out[i];
    if (o.call_ms) *o.call_ms = ms;
    *o.ret = mono[i]; *o.desc_rows = desc[i].rows;
    tokens[i] = extractors[i]->mnPyramidToken;
    PutPyramid(*extractors[i], in[i].nlevels, o);
    if (mono[i] < 0) continue;   // an empty image: the extractor's outputs were not touched
    if (!PutKeypoints(keys[i], desc[i], o)) return -1;
  }
  return 0;
}
