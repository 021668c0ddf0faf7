// orb_pyramid.h -- ORBextractor::ComputePyramid (src/ORBextractor.cc:1170-1195) restated from the definitions: the level sizes, the
// cv::resize(..., INTER_LINEAR) of a CV_8UC1 level from the level before it, and the copyMakeBorder(BORDER_REFLECT_101) around it.
// Device code of orb_pyramid_device.hip; plain C++ as well, so the test library and `make pyramid-check` run the same statements on
// the host.
//
// The resampling is DEFINED HERE (include/orbslam3_hip.h states it in full): it is OpenCV's 8-bit fixed-point path as recalled, not
// verified against OpenCV, so parity with cv::resize is unpinned.
//   sizes    cols_l = cvRound((float)cols_0 * inv_scale[l]), rows likewise, always from level 0; halves to even
//   tables   per (src, dst) and axis, on the host only: scale = 1.0 / ((double)dst / (double)src), f = (float)((d + 0.5) * scale - 0.5),
//            s = floor(f), f -= s in float32; columns clamp (s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0), rows keep f and
//            clamp the two row indices; w0 = cvRound((1.f - f) * 2048.f), w1 = cvRound(f * 2048.f) as int16
//   pixel    h_r = S[r][sx] * a0 + S[r][sx + 1] * a1; out = (uint8)((((b0 * (h_0 >> 4)) >> 16) + ((b1 * (h_1 >> 4)) >> 16) + 2) >> 2)
//   halving  src == 2 * dst in both axes: out = (S[2y][2x] + S[2y][2x+1] + S[2y+1][2x] + S[2y+1][2x+1] + 2) >> 2
//   border   reflect-101 repeated as often as needed (pyr_reflect101; brief_reflect101 of orb_brief.h has a narrower domain)
// The device never computes a table entry: the tables are input data of the launch and the kernels are integer only.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orb_fast.h"

namespace osh {

constexpr int kPyrEdge = 19;   // EDGE_THRESHOLD: the border ComputePyramid leaves around every level

// One destination index of one axis: the two source indices and their Q11 weights.  For a column s1 = min(s0 + 1, src - 1); where
// the definition does not read the second tap its weight is 0.
struct PyrTap { int32_t s0, s1; int16_t w0, w1; };

// Side of level l for a level 0 of `size0` pixels
inline int pyr_level_size(int size0, float inv_scale) {
#pragma clang fp contract(off)
  const float v = (float)size0 * inv_scale;
  if (!(v >= -1.f && v <= 1.0e9f)) return v > 0.f ? 1 << 30 : 0;   // beyond every supported side: kept out of the conversion
  return fast_cv_round(v);
}

// The table of one axis: `dst` entries.  rows: the row rule (f kept, indices clamped), else the column rule.
inline void pyr_axis_table(int src, int dst, bool rows, PyrTap* out) {
#pragma clang fp contract(off)
  const double scale = 1.0 / ((double)dst / (double)src);
  for (int d = 0; d < dst; ++d) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)std::floor(f);
    f -= (float)s;
    PyrTap t;
    if (rows) {
      t.s0 = fast_min(fast_max(s, 0), src - 1);
      t.s1 = fast_min(fast_max(s + 1, 0), src - 1);
    } else {
      if (s < 0) { s = 0; f = 0.f; }
      if (s >= src - 1) { s = src - 1; f = 0.f; }
      t.s0 = s;
      t.s1 = fast_min(s + 1, src - 1);
    }
    t.w0 = (int16_t)fast_cv_round((1.f - f) * 2048.f);
    t.w1 = (int16_t)fast_cv_round(f * 2048.f);
    out[d] = t;
  }
}

// Whether (src -> dst) takes the exact-halving path
OSH_FAST_HD bool pyr_is_halving(int src_rows, int src_cols, int dst_rows, int dst_cols) {
  return src_cols == 2 * dst_cols && src_rows == 2 * dst_rows;
}

// One pixel from the two source rows r0, r1 (already selected by the row tap), the column tap cx and the row weights
OSH_FAST_HD uint8_t pyr_pixel(const uint8_t* r0, const uint8_t* r1, const PyrTap& cx, int b0, int b1) {
  const int h0 = (int)r0[cx.s0] * cx.w0 + (int)r0[cx.s1] * cx.w1;
  const int h1 = (int)r1[cx.s0] * cx.w0 + (int)r1[cx.s1] * cx.w1;
  return (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}
// One pixel of the exact-halving path from source rows 2y and 2y + 1
OSH_FAST_HD uint8_t pyr_half_pixel(const uint8_t* r0, const uint8_t* r1, int x) {
  return (uint8_t)(((int)r0[2 * x] + (int)r0[2 * x + 1] + (int)r1[2 * x] + (int)r1[2 * x + 1] + 2) >> 2);
}

// BORDER_REFLECT_101 for any p: m = p mod 2 (len - 1), m when m < len, else 2 (len - 1) - m; len == 1 gives 0
OSH_FAST_HD int pyr_reflect101(int p, int len) {
  if (len == 1) return 0;
  const int period = 2 * (len - 1);
  int m = p % period;
  if (m < 0) m += period;
  return m < len ? m : period - m;
}

// ---- host only: whole levels, as the kernels of orb_pyramid_device.hip do them

// Level (dst_rows x dst_cols, rows dst_stride apart) from the level before it
inline void pyr_resample_level_host(const uint8_t* src, int src_rows, int src_cols, long long src_stride, uint8_t* dst, int dst_rows, int dst_cols,
                                    long long dst_stride) {
  if (pyr_is_halving(src_rows, src_cols, dst_rows, dst_cols)) {
    for (int y = 0; y < dst_rows; ++y)
      for (int x = 0; x < dst_cols; ++x) dst[y * dst_stride + x] = pyr_half_pixel(src + 2 * y * src_stride, src + (2 * y + 1) * src_stride, x);
    return;
  }
  std::vector<PyrTap> cx((size_t)dst_cols), ry((size_t)dst_rows);
  pyr_axis_table(src_cols, dst_cols, false, cx.data());
  pyr_axis_table(src_rows, dst_rows, true, ry.data());
  for (int y = 0; y < dst_rows; ++y) {
    const uint8_t* r0 = src + ry[y].s0 * src_stride;
    const uint8_t* r1 = src + ry[y].s1 * src_stride;
    for (int x = 0; x < dst_cols; ++x) dst[y * dst_stride + x] = pyr_pixel(r0, r1, cx[x], ry[y].w0, ry[y].w1);
  }
}

// The `border` pixels around a level whose first pixel is `level` inside a larger image (rows `stride` apart): every pixel outside
// the level from the level by reflect-101
inline void pyr_border_host(uint8_t* level, int rows, int cols, long long stride, int border) {
  for (int y = -border; y < rows + border; ++y)
    for (int x = -border; x < cols + border; ++x)
      if (y < 0 || y >= rows || x < 0 || x >= cols) level[y * stride + x] = level[pyr_reflect101(y, rows) * stride + pyr_reflect101(x, cols)];
}

}  // namespace osh
