// orb_prepare.h -- what the reference does to a camera image before ORBextractor::operator() reads it, restated from the definitions:
// the cv::remap(..., INTER_LINEAR) of System::TrackStereo (src/System.cc:252-269) with the CV_32F maps of
// Settings::precomputeRectificationMaps, the cv::resize of TrackStereo / TrackRGBD / TrackMonocular, and the cvtColor(.., *2GRAY) of
// Tracking::GrabImage* (src/Tracking.cc:1462-1489, :1524-1538, :1568-1582).  Device code of orb_prepare_device.hip; plain C++ as well,
// so the test library and `make prepare-check` run the same statements on the host.
//
// The three steps are DEFINED HERE (include/orbslam3_hip.h states them in full): they are OpenCV's 8-bit paths as recalled, not
// verified against OpenCV, so parity with cv::remap, cv::resize and cv::cvtColor is unpinned.
//   order    the reference's: geometry first, on every channel, then grey
//   remap    mx = map_x[y][x], my = map_y[y][x] (float32); a coordinate is usable when it is finite and |m| <= 32768; an unusable one
//            makes the pixel 0 in every channel; sx = cvRound(mx * 32.f) (the product is exact, halves to even), ix = sx >> 5,
//            fx = sx & 31, sy / iy / fy likewise; per channel, with p(r, c) = 0 outside the source, tap by tap,
//            out = ((32 - fy) * ((32 - fx) * p(iy, ix) + fx * p(iy, ix + 1)) + fy * ((32 - fx) * p(iy + 1, ix) + fx * p(iy + 1, ix + 1)) + 512) >> 10
//   resize   per channel pyr_axis_table / pyr_pixel / pyr_half_pixel of orb_pyramid.h from the input size to the output size
//   grey     1 channel: the value; 3 or 4: Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14, a fourth channel is ignored
// The device computes no table entry; apart from mx * 32.f and its conversion the kernel is integer only.
#pragma once
#include <cstdint>
#include <vector>

#include "orb_pyramid.h"

namespace osh {

constexpr int kPrepRGB = 0, kPrepBGR = 1;          // OSH_PREP_RGB, OSH_PREP_BGR
constexpr int kPrepPass = 0, kPrepRemap = 1, kPrepResize = 2, kPrepHalve = 3;   // what a frame's geometry step is

// The interleaved source image of a frame: `channels` bytes per pixel, rows `stride` bytes apart
struct PrepSource {
  const uint8_t* data;
  long long stride;
  int rows, cols, channels, bgr;
};

// Tested before the conversion: what cvRound makes of a NaN or of a float beyond the int range is not what the definition says
OSH_FAST_HD bool prep_usable(float m) { return m >= -32768.f && m <= 32768.f; }   // false for a NaN

OSH_FAST_HD int prep_q5(float m) {
#pragma clang fp contract(off)
  return fast_cv_round(m * 32.f);
}

OSH_FAST_HD uint8_t prep_gray(int r, int g, int b) { return (uint8_t)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14); }

// Grey of the `channels` values at v (the geometry step's result for one pixel)
OSH_FAST_HD uint8_t prep_gray_of(const int* v, int channels, int bgr) {
  if (channels == 1) return (uint8_t)v[0];
  return bgr ? prep_gray(v[2], v[1], v[0]) : prep_gray(v[0], v[1], v[2]);
}

// p(r, c) of channel ch: 0 outside the source
OSH_FAST_HD int prep_tap(const PrepSource& S, int r, int c, int ch) {
  return (r >= 0 && r < S.rows && c >= 0 && c < S.cols) ? (int)S.data[(long long)r * S.stride + (long long)c * S.channels + ch] : 0;
}

// One destination pixel of a frame with a map
OSH_FAST_HD uint8_t prep_remap_pixel(const PrepSource& S, float mx, float my) {
  if (!prep_usable(mx) || !prep_usable(my)) return 0;   // 0 in every channel: grey 0
  const int sx = prep_q5(mx), sy = prep_q5(my);
  const int ix = sx >> 5, fx = sx & 31, iy = sy >> 5, fy = sy & 31;
  int v[3] = {0, 0, 0};
  const int nc = S.channels == 1 ? 1 : 3;
  for (int ch = 0; ch < nc; ++ch) {
    const int top = (32 - fx) * prep_tap(S, iy, ix, ch) + fx * prep_tap(S, iy, ix + 1, ch);
    const int bottom = (32 - fx) * prep_tap(S, iy + 1, ix, ch) + fx * prep_tap(S, iy + 1, ix + 1, ch);
    v[ch] = ((32 - fy) * top + fy * bottom + 512) >> 10;
  }
  return prep_gray_of(v, S.channels, S.bgr);
}

// One destination pixel of a resized frame from the row tap ry and the column tap cx (the tables of orb_pyramid.h for the two sizes):
// the four source values of a channel side by side, so that pyr_pixel itself makes the pixel
OSH_FAST_HD uint8_t prep_resize_pixel(const PrepSource& S, const PyrTap& ry, const PyrTap& cx) {
  const uint8_t* r0 = S.data + (long long)ry.s0 * S.stride;
  const uint8_t* r1 = S.data + (long long)ry.s1 * S.stride;
  PyrTap pair = cx;
  pair.s0 = 0; pair.s1 = 1;
  int v[3] = {0, 0, 0};
  const int nc = S.channels == 1 ? 1 : 3;
  for (int ch = 0; ch < nc; ++ch) {
    const uint8_t a[2] = {r0[(long long)cx.s0 * S.channels + ch], r0[(long long)cx.s1 * S.channels + ch]};
    const uint8_t b[2] = {r1[(long long)cx.s0 * S.channels + ch], r1[(long long)cx.s1 * S.channels + ch]};
    v[ch] = pyr_pixel(a, b, pair, ry.w0, ry.w1);
  }
  return prep_gray_of(v, S.channels, S.bgr);
}

// One destination pixel (y, x) of a frame that is halved exactly: pyr_half_pixel on the four source values of a channel
OSH_FAST_HD uint8_t prep_halve_pixel(const PrepSource& S, int y, int x) {
  const uint8_t* r0 = S.data + (long long)(2 * y) * S.stride + (long long)(2 * x) * S.channels;
  const uint8_t* r1 = r0 + S.stride;
  int v[3] = {0, 0, 0};
  const int nc = S.channels == 1 ? 1 : 3;
  for (int ch = 0; ch < nc; ++ch) {
    const uint8_t a[2] = {r0[ch], r0[S.channels + ch]};
    const uint8_t b[2] = {r1[ch], r1[S.channels + ch]};
    v[ch] = pyr_half_pixel(a, b, 0);
  }
  return prep_gray_of(v, S.channels, S.bgr);
}

// One pixel of a frame whose size stays and that has no map
OSH_FAST_HD uint8_t prep_pass_pixel(const PrepSource& S, int y, int x) {
  const uint8_t* p = S.data + (long long)y * S.stride + (long long)x * S.channels;
  int v[3] = {p[0], 0, 0};
  if (S.channels != 1) { v[1] = p[1]; v[2] = p[2]; }
  return prep_gray_of(v, S.channels, S.bgr);
}

// The geometry step of a frame without a map
inline int prep_mode(int src_rows, int src_cols, int dst_rows, int dst_cols) {
  if (src_rows == dst_rows && src_cols == dst_cols) return kPrepPass;
  return pyr_is_halving(src_rows, src_cols, dst_rows, dst_cols) ? kPrepHalve : kPrepResize;
}

// ---- host only: a whole frame, as k_prepare of orb_prepare_device.hip does it

// The grey image (dst_rows x dst_cols, rows dst_stride apart).  With a map (map_x != nullptr; rows of floats map_stride BYTES apart)
// the destination size is the map's; without one the source is resized when the sizes differ
inline void prep_frame_host(const PrepSource& S, const float* map_x, long long map_x_stride, const float* map_y, long long map_y_stride, uint8_t* dst,
                            int dst_rows, int dst_cols, long long dst_stride) {
  if (map_x) {
    for (int y = 0; y < dst_rows; ++y) {
      const float* mx = reinterpret_cast<const float*>(reinterpret_cast<const char*>(map_x) + y * map_x_stride);
      const float* my = reinterpret_cast<const float*>(reinterpret_cast<const char*>(map_y) + y * map_y_stride);
      for (int x = 0; x < dst_cols; ++x) dst[y * dst_stride + x] = prep_remap_pixel(S, mx[x], my[x]);
    }
    return;
  }
  const int mode = prep_mode(S.rows, S.cols, dst_rows, dst_cols);
  std::vector<PyrTap> cx, ry;
  if (mode == kPrepResize) {
    cx.resize((size_t)dst_cols); ry.resize((size_t)dst_rows);
    pyr_axis_table(S.cols, dst_cols, false, cx.data());
    pyr_axis_table(S.rows, dst_rows, true, ry.data());
  }
  for (int y = 0; y < dst_rows; ++y)
    for (int x = 0; x < dst_cols; ++x)
      dst[y * dst_stride + x] = mode == kPrepPass ? prep_pass_pixel(S, y, x) : mode == kPrepHalve ? prep_halve_pixel(S, y, x) : prep_resize_pixel(S, ry[y], cx[x]);
}

}  // namespace osh
