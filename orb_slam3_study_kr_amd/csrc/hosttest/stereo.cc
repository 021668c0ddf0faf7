// stereo.cc -- osh_host_pack_stereo / osh_host_compute_stereo_matches / osh_host_stereo_restatement (include/orbslam3_hip_host.h):
// Frame::ComputeStereoMatches and its pack on a stand-in Frame built from flat arrays, whose pyramid levels are views into bordered
// images like the reference's, and a plain single-thread C++ restatement of src/Frame.cc:816-986 (the CPU baseline of
// profiles/stereo_timing.py and the checker of long runs).  osh_host_compute_fisheye_stereo_matches drives
// Frame::ComputeStereoFishEyeMatches on a stand-in rig Frame; osh_host_kb8_triangulate_cpu runs the device's
// csrc/kb8_triangulate.h on the host.  Test library only.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Frame.h"
#include "ORBextractor.h"
#include "host_pack.h"
#include "../kb8_triangulate.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

using namespace ORB_SLAM3;

namespace {

struct StereoScene {
  Frame F;
  ORBextractor left, right;
};

bool usable(const osh_host_stereo_input* in) {
  return in && in->n_left >= 0 && in->n_right >= 0 && in->n_levels >= 1 && in->scale_factors && in->inv_scale_factors &&
         in->left_rows && in->left_cols && in->right_rows && in->right_cols && in->left_pixels && in->right_pixels;
}

// a pyramid whose level l is a view into an image with `border` pixels around it, filled with a value the level itself never shows
// through the pack (167), so that a walk by `cols` instead of `step` cannot go unnoticed
void build_pyramid(std::vector<cv::Mat>& pyr, int n_levels, const int32_t* rows, const int32_t* cols, const uint8_t* pixels, int border) {
  pyr.resize(n_levels);
  size_t off = 0;
  for (int l = 0; l < n_levels; ++l) {
    cv::Mat whole(rows[l] + 2 * border, cols[l] + 2 * border);
    for (int r = 0; r < whole.rows; ++r) std::memset(whole.ptr<uint8_t>(r), 167, (size_t)whole.cols);
    pyr[l] = whole.view(border, border, rows[l], cols[l]);
    for (int r = 0; r < rows[l]; ++r) std::memcpy(pyr[l].ptr<uint8_t>(r), pixels + off + (size_t)r * cols[l], (size_t)cols[l]);
    off += (size_t)rows[l] * cols[l];
  }
}

void build(const osh_host_stereo_input* in, int border, StereoScene& sc) {
  Frame& F = sc.F;
  auto keys = [](int n, const float* xy, const int32_t* oct, const uint8_t* desc, std::vector<cv::KeyPoint>& k, cv::Mat& D) {
    k.resize(n);
    D = cv::Mat(n, 32);
    for (int i = 0; i < n; ++i) {
      k[i].pt.x = xy[2 * i]; k[i].pt.y = xy[2 * i + 1]; k[i].octave = oct[i];
      std::memcpy(D.ptr<uint8_t>(i), desc + 32 * (size_t)i, 32);
    }
  };
  keys(in->n_left, in->left_xy, in->left_octave, in->left_desc, F.mvKeys, F.mDescriptors);
  keys(in->n_right, in->right_xy, in->right_octave, in->right_desc, F.mvKeysRight, F.mDescriptorsRight);
  F.N = in->n_left;
  F.mvScaleFactors.assign(in->scale_factors, in->scale_factors + in->n_levels);
  F.mvInvScaleFactors.assign(in->inv_scale_factors, in->inv_scale_factors + in->n_levels);
  F.mnScaleLevels = in->n_levels;
  F.mbf = in->bf; F.mb = in->b;
  build_pyramid(sc.left.mvImagePyramid, in->n_levels, in->left_rows, in->left_cols, in->left_pixels, border);
  build_pyramid(sc.right.mvImagePyramid, in->n_levels, in->right_rows, in->right_cols, in->right_pixels, border);
  F.mpORBextractorLeft = &sc.left;
  F.mpORBextractorRight = &sc.right;
}

inline int hamming256(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int k = 0; k < 4; ++k) {
    uint64_t x, y;
    std::memcpy(&x, a + 8 * k, 8); std::memcpy(&y, b + 8 * k, 8);
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}

}  // namespace

extern "C" int osh_host_pack_stereo(const osh_host_stereo_input* in, int32_t border, int32_t sizes[3], float* left_xy, int32_t* left_octave,
                                    uint8_t* left_desc, float* right_xy, int32_t* right_octave, uint8_t* right_desc, float* scales,
                                    int64_t* level_shape, uint8_t* left_pixels, uint8_t* right_pixels, float bf_b[2]) {
  if (!usable(in) || border < 0) return -1;
  StereoScene sc;
  build(in, border, sc);
  StereoPack pk;
  if (!PackStereoMatches(sc.F, pk)) return -2;
  osh_stereo_frame f;
  pk.fill(f, sc.F);
  if (sizes) { sizes[0] = f.n_left; sizes[1] = f.n_right; sizes[2] = f.n_levels; }
  if (left_xy) std::memcpy(left_xy, f.left_xy, (size_t)f.n_left * 8);
  if (left_octave) std::memcpy(left_octave, f.left_octave, (size_t)f.n_left * 4);
  if (left_desc) std::memcpy(left_desc, f.left_desc, (size_t)f.n_left * 32);
  if (right_xy) std::memcpy(right_xy, f.right_xy, (size_t)f.n_right * 8);
  if (right_octave) std::memcpy(right_octave, f.right_octave, (size_t)f.n_right * 4);
  if (right_desc) std::memcpy(right_desc, f.right_desc, (size_t)f.n_right * 32);
  if (scales) for (int l = 0; l < f.n_levels; ++l) { scales[2 * l] = f.scale_factors[l]; scales[2 * l + 1] = f.inv_scale_factors[l]; }
  if (bf_b) { bf_b[0] = f.bf; bf_b[1] = f.b; }
  const osh_stereo_image* pyr[2] = {f.left_pyramid, f.right_pyramid};
  uint8_t* px[2] = {left_pixels, right_pixels};
  for (int side = 0; side < 2; ++side) {
    size_t off = 0;
    for (int l = 0; l < f.n_levels; ++l) {
      const osh_stereo_image& im = pyr[side][l];
      if (level_shape) { int64_t* s = level_shape + ((size_t)side * f.n_levels + l) * 3; s[0] = im.rows; s[1] = im.cols; s[2] = im.stride; }
      // the walk a consumer of osh_stereo_image makes: row r starts at data + r * stride
      if (px[side]) for (int r = 0; r < im.rows; ++r) std::memcpy(px[side] + off + (size_t)r * im.cols, im.data + (size_t)r * im.stride, (size_t)im.cols);
      off += (size_t)im.rows * im.cols;
    }
  }
  return 0;
}

extern "C" int osh_host_compute_stereo_matches(const osh_host_stereo_input* in, int32_t border, float* u_right, float* depth) {
  if (!usable(in) || border < 0 || !u_right || !depth) return -1;
  StereoScene sc;
  build(in, border, sc);
  sc.F.ComputeStereoMatches();
  if ((int)sc.F.mvuRight.size() != in->n_left || (int)sc.F.mvDepth.size() != in->n_left) return -2;
  std::copy(sc.F.mvuRight.begin(), sc.F.mvuRight.end(), u_right);
  std::copy(sc.F.mvDepth.begin(), sc.F.mvDepth.end(), depth);
  return 0;
}

// The steps of src/Frame.cc:816-986 in one thread, on the contiguous levels of the input.  The four places where the reference's
// behaviour is undefined are defined skips, counted in undefined[4]: [0] row-table entries outside [0, nRows), [1] left keypoints whose
// row is outside, [2] keypoints whose patches leave their image, [3] 1 if no keypoint was accepted (no median).
extern "C" int osh_host_stereo_restatement(const osh_host_stereo_input* in, float* u_right, float* depth, int32_t* best_right, int32_t* hamming,
                                           int32_t* sad, int32_t* best_inc, uint8_t* stage, uint8_t* flags, int32_t undefined[4], double* ms) {
#pragma clang fp contract(off)
  if (!usable(in) || !u_right || !depth) return -1;
  const auto t0 = std::chrono::steady_clock::now();
  const int N = in->n_left, Nr = in->n_right, nRows = in->left_rows[0];
  int undef[4] = {0, 0, 0, 0};
  std::vector<size_t> off_l(in->n_levels), off_r(in->n_levels);
  { size_t a = 0, b = 0; for (int l = 0; l < in->n_levels; ++l) { off_l[l] = a; off_r[l] = b; a += (size_t)in->left_rows[l] * in->left_cols[l]; b += (size_t)in->right_rows[l] * in->right_cols[l]; } }
  // step 1: row table
  std::vector<std::vector<int>> rows(std::max(nRows, 0));
  for (int iR = 0; iR < Nr; ++iR) {
    const float y = in->right_xy[2 * iR + 1];
    const float r = 2.0f * in->scale_factors[in->right_octave[iR]];
    const int maxr = (int)std::ceil(y + r), minr = (int)std::floor(y - r);
    for (int yi = minr; yi <= maxr; ++yi) { if (yi < 0 || yi >= nRows) { ++undef[0]; continue; } rows[yi].push_back(iR); }
  }
  const float maxD = in->bf / in->b;
  std::vector<int> acc_sad, acc_idx;
  for (int iL = 0; iL < N; ++iL) {
    const float uL = in->left_xy[2 * iL], vL = in->left_xy[2 * iL + 1];
    const int levelL = in->left_octave[iL];
    int st = -1, br = -1, ham = -1, binc = OSH_STEREO_NO_INC, fl = 0;
    int sads[11]; for (int k = 0; k < 11; ++k) sads[k] = -1;
    float ur = -1.0f, dp = -1.0f;
    const int row = (int)vL;
    const bool row_in = row >= 0 && row < nRows;
    if (!row_in) ++undef[1];
    if (!row_in || rows[row].empty() || uL - 0.0f < 0) {
      st = OSH_STEREO_NO_CANDIDATE;
    } else {
      // step 2
      const float minU = uL - maxD, maxU = uL - 0.0f;
      ham = 100;
      for (int iR : rows[row]) {
        const int o = in->right_octave[iR];
        if (o < levelL - 1 || o > levelL + 1) continue;
        const float uR = in->right_xy[2 * iR];
        if (uR >= minU && uR <= maxU) {
          const int d = hamming256(in->left_desc + 32 * (size_t)iL, in->right_desc + 32 * (size_t)iR);
          if (d < ham) { ham = d; br = iR; }
        }
      }
      if (!(ham < 75)) {
        st = OSH_STEREO_HAMMING;
      } else {
        // step 3
        const float isf = in->inv_scale_factors[levelL];
        const float su = std::round(uL * isf), sv = std::round(vL * isf), sr = std::round(in->right_xy[2 * br] * isf);
        const int cl = in->left_cols[levelL], rl = in->left_rows[levelL], cr = in->right_cols[levelL], rr = in->right_rows[levelL];
        const int iu = (int)su, iv = (int)sv, ir = (int)sr;
        if (sr < 0 || sr + 11.0f >= (float)cr) {
          st = OSH_STEREO_RIGHT_GUARD;
        } else if (iv - 5 < 0 || iv + 5 >= rl || iv + 5 >= rr || iu - 5 < 0 || iu + 5 >= cl || ir - 10 < 0 || ir + 10 >= cr) {
          st = OSH_STEREO_PATCH; ++undef[2];
        } else {
          const uint8_t* L = in->left_pixels + off_l[levelL];
          const uint8_t* R = in->right_pixels + off_r[levelL];
          int best = INT_MAX, n_min = 0;
          for (int inc = -5; inc <= 5; ++inc) {
            int s = 0;
            for (int y = -5; y <= 5; ++y) {
              const uint8_t* a = L + (size_t)(iv + y) * cl + (iu - 5);
              const uint8_t* b = R + (size_t)(iv + y) * cr + (ir + inc - 5);
              for (int x = 0; x < 11; ++x) s += std::abs((int)a[x] - (int)b[x]);
            }
            sads[inc + 5] = s;
            if (s < best) { best = s; binc = inc; n_min = 1; } else if (s == best) ++n_min;
          }
          if (n_min > 1) fl |= 2;
          if (binc == -5 || binc == 5) {
            st = OSH_STEREO_BORDER_INC;
          } else {
            // step 4
            const float d1 = (float)sads[5 + binc - 1], d2 = (float)sads[5 + binc], d3 = (float)sads[5 + binc + 1];
            const float delta = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2));
            if (delta < -1 || delta > 1) {
              st = OSH_STEREO_DELTA;
            } else {
              float bu = in->scale_factors[levelL] * ((float)ir + (float)binc + delta);
              float disp = uL - bu;
              if (disp >= 0.0f && disp < maxD) {
                if (disp <= 0) { disp = 0.01f; bu = (float)((double)uL - 0.01); fl |= 1; }
                dp = in->bf / disp; ur = bu;
                st = OSH_STEREO_ACCEPTED;
                acc_sad.push_back(best); acc_idx.push_back(iL);
              } else {
                st = OSH_STEREO_DISPARITY;
              }
            }
          }
        }
      }
    }
    u_right[iL] = ur; depth[iL] = dp;
    if (best_right) best_right[iL] = br;
    if (hamming) hamming[iL] = ham;
    if (sad) std::memcpy(sad + 11 * (size_t)iL, sads, sizeof sads);
    if (best_inc) best_inc[iL] = binc;
    if (stage) stage[iL] = (uint8_t)st;
    if (flags) flags[iL] = (uint8_t)fl;
  }
  // step 5: only the value of the size/2-th smallest accepted SAD matters
  if (acc_sad.empty()) {
    undef[3] = 1;
  } else {
    std::vector<int> sorted(acc_sad);
    std::nth_element(sorted.begin(), sorted.begin() + sorted.size() / 2, sorted.end());
    const float median = (float)sorted[sorted.size() / 2];
    const float th = 1.5f * 1.4f * median;
    for (size_t k = 0; k < acc_sad.size(); ++k)
      if (!((float)acc_sad[k] < th)) {
        u_right[acc_idx[k]] = -1.0f; depth[acc_idx[k]] = -1.0f;
        if (stage) stage[acc_idx[k]] = OSH_STEREO_MEDIAN_CUT;
      }
  }
  if (undefined) for (int k = 0; k < 4; ++k) undefined[k] = undef[k];
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// ---- Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1131-1171)
extern "C" int osh_host_compute_fisheye_stereo_matches(const osh_host_fisheye_input* in, int32_t camera2_pinhole, int32_t* left_to_right,
                                                       int32_t* right_to_left, float* depth, float* p3d, float* u_right) {
  if (!in || in->n_left < 0 || in->n_right < 0 || in->n_levels < 0) return -1;
  Frame F;
  auto keys = [](int n, const float* xy, const int32_t* oct, const uint8_t* desc, std::vector<cv::KeyPoint>& k, cv::Mat& D) {
    k.resize(n);
    D = cv::Mat(n, 32);
    for (int i = 0; i < n; ++i) {
      k[i].pt.x = xy[2 * i]; k[i].pt.y = xy[2 * i + 1]; k[i].octave = oct[i];
      std::memcpy(D.ptr<uint8_t>(i), desc + 32 * (size_t)i, 32);
    }
  };
  keys(in->n_left, in->left_xy, in->left_octave, in->left_desc, F.mvKeys, F.mDescriptors);
  keys(in->n_right, in->right_xy, in->right_octave, in->right_desc, F.mvKeysRight, F.mDescriptorsRight);
  F.Nleft = in->n_left; F.Nright = in->n_right; F.N = in->n_left + in->n_right;
  F.monoLeft = in->mono_left; F.monoRight = in->mono_right;
  if (in->n_levels) F.mvLevelSigma2.assign(in->level_sigma2, in->level_sigma2 + in->n_levels);
  F.mnScaleLevels = in->n_levels;
  KannalaBrandt8 cam1(std::vector<float>(in->cam1, in->cam1 + 8), in->precision1), cam2(std::vector<float>(in->cam2, in->cam2 + 8), in->precision2);
  Pinhole pin(std::vector<float>(in->cam2, in->cam2 + 4));
  F.mpCamera = &cam1;
  F.mpCamera2 = camera2_pinhole ? static_cast<GeometricCamera*>(&pin) : &cam2;
  Eigen::Matrix3f Rlr; Eigen::Vector3f tlr;
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rlr(r, c) = in->Rlr[3 * r + c]; tlr(r) = in->tlr[r]; }
  F.SetRelativePoseTlr(Rlr, tlr);   // :1102-1105
  F.ComputeStereoFishEyeMatches();
  const size_t nl = (size_t)in->n_left, nr = (size_t)in->n_right;
  if (F.mvLeftToRightMatch.size() != nl || F.mvRightToLeftMatch.size() != nr || F.mvDepth.size() != nl || F.mvStereo3Dpoints.size() != nl ||
      F.mvuRight.size() != nl) return -2;
  if (left_to_right) std::copy(F.mvLeftToRightMatch.begin(), F.mvLeftToRightMatch.end(), left_to_right);
  if (right_to_left) std::copy(F.mvRightToLeftMatch.begin(), F.mvRightToLeftMatch.end(), right_to_left);
  if (depth) std::copy(F.mvDepth.begin(), F.mvDepth.end(), depth);
  if (u_right) std::copy(F.mvuRight.begin(), F.mvuRight.end(), u_right);
  if (p3d) for (size_t i = 0; i < nl; ++i) for (int k = 0; k < 3; ++k) p3d[3 * i + k] = F.mvStereo3Dpoints[i](k);
  return 0;
}

extern "C" int osh_host_kb8_triangulate_cpu(int32_t n, const osh_kb8_rig* rig, const float* xy1, const float* xy2, const float* sigma1,
                                            const float* sigma2, float* ret, float* p3d, float* cos_parallax) {
  if (n < 0 || !rig || (n && (!xy1 || !xy2 || !sigma1 || !sigma2 || !ret || !p3d || !cos_parallax))) return -1;
  osh::Kb8Rig g;
  std::memcpy(g.cam1, rig->cam1, sizeof g.cam1); std::memcpy(g.cam2, rig->cam2, sizeof g.cam2);
  g.prec1 = rig->precision1; g.prec2 = rig->precision2;
  std::memcpy(g.R12, rig->R12, sizeof g.R12); std::memcpy(g.t12, rig->t12, sizeof g.t12);
  for (int i = 0; i < n; ++i)
    ret[i] = osh::kb8_triangulate_match(g, xy1[2 * i], xy1[2 * i + 1], xy2[2 * i], xy2[2 * i + 1], sigma1[i], sigma2[i], p3d + 3 * (size_t)i, cos_parallax + i);
  return 0;
}
