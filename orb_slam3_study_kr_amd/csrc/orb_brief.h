// orb_brief.h -- what ORBextractor::operator() (src/ORBextractor.cc:1086-1168) does per level after ComputeKeyPointsOctTree, restated
// from definitions: a 7x7 separable Gaussian blur of the level in integers, and the 256 rotated intensity comparisons of
// computeOrbDescriptor (:107-146) per keypoint.  Device code of orb_brief_device.hip; plain C++ as well, so the test library and
// `make brief-check` run the same statements on the host.
//
// Blur of a level of rows x cols bytes with the Q8 weights w[0..6] (sum 256), r(i, n) the reflect-101 index:
//   h(y, x) = sum_u w[u] * I(y, r(x + u - 3, cols))                       exact, at most 255 * 256 = 65280: 16 bits
//   B(y, x) = (sum_v w[v] * h(r(y + v - 3, rows), x) + 32768) >> 16       at most 256 * 65280 + 32768 < 2^31; one rounding
// Integers throughout: the order of the sums is free.  r is defined for n >= 4 (a 3-pixel halo reflects into the level).
//
// Descriptor of a keypoint (x, y, angle in degrees) on the blurred level, with the 512 points p of the sampling table as input data:
//   rad = angle * factorPI (one float32 product), a = (float)cos((double)rad), b = (float)sin((double)rad);
//   sample(p) = B[cvRound(y) + cvRound(p.x * b + p.y * a)][cvRound(x) + cvRound(p.x * a - p.y * b)], two float32 products and one
//   float32 sum or difference, never fused, cvRound to nearest with halves to even;
//   bit k of byte i = sample(point 16 i + 2 k) < sample(point 16 i + 2 k + 1).
#pragma once
#include "orb_fast.h"

namespace osh {

constexpr int kBriefTaps = 7;
constexpr int kBriefHalo = 3;
constexpr int kBriefPoints = 512;         // of the table; x and y interleaved: 1024 int8
constexpr int kBriefMaxCoord = 15;        // HALF_PATCH_SIZE: |p.x|, |p.y| <= 15, so the reach is at most 22
constexpr int kBriefMinSide = 4;          // the smallest level side the blur is defined for

// BORDER_REFLECT_101: -i for i < 0, 2 (n - 1) - i for i >= n; needs -(n - 1) <= i <= 2 (n - 1)
OSH_FAST_HD int brief_reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

// h(y, x) for the row at `row`
OSH_FAST_HD int brief_blur_h(const uint8_t* row, int x, int cols, const uint16_t* w) {
  int acc = 0;
#pragma unroll
  for (int u = 0; u < kBriefTaps; ++u) acc += (int)w[u] * row[brief_reflect101(x + u - kBriefHalo, cols)];
  return acc;
}
// the single rounding of B from the vertical sum
OSH_FAST_HD uint8_t brief_blur_round(int acc) { return (uint8_t)((acc + 32768) >> 16); }

struct BriefRot { float a, b; };   // cos, sin of the keypoint's angle
OSH_FAST_HD BriefRot brief_rotation(float angle_deg) {
#pragma clang fp contract(off)
  const float factor_pi = (float)(3.14159265358979323846 / 180.0);
  const float rad = angle_deg * factor_pi;
  BriefRot r;
  r.a = (float)cos((double)rad);
  r.b = (float)sin((double)rad);
  return r;
}
// the rounded offset of table point (px, py): dx along the row, dy across rows
OSH_FAST_HD void brief_offset(BriefRot r, int px, int py, int& dx, int& dy) {
#pragma clang fp contract(off)
  const float fx = (float)px, fy = (float)py;
  const float xa = fx * r.a, yb = fy * r.b, xb = fx * r.b, ya = fy * r.a;
  dx = fast_cv_round(xa - yb);
  dy = fast_cv_round(xb + ya);
}
// pair j of the table (points 2 j and 2 j + 1) around the pixel at `centre` of the blurred level
template <class Pitch>
OSH_FAST_HD bool brief_pair(const uint8_t* centre, Pitch pitch, BriefRot r, const int8_t* pattern, int j) {
  int dx0, dy0, dx1, dy1;
  brief_offset(r, pattern[4 * j], pattern[4 * j + 1], dx0, dy0);
  brief_offset(r, pattern[4 * j + 2], pattern[4 * j + 3], dx1, dy1);
  return centre[dy0 * pitch + dx0] < centre[dy1 * pitch + dx1];
}

// Reach of a table: R = ceil(max sqrt(p.x^2 + p.y^2)), the largest distance in pixels a sample can lie from the keypoint's pixel
// in either direction.  A rounded offset never exceeds R: the exact offset is a coordinate of p rotated, so its magnitude is at most
// r = |p| <= R, and cvRound only passes R from a value of at least R + 0.5.  The float32 form (two products and a sum of values
// below 32, a and b within 1e-7 of a unit vector) errs by less than 1e-5, nowhere near the 0.5 of margin.  The same holds one
// pixel tighter, which is why the real table (r up to 18.38) needs 19 and not 20: r^2 is an integer, (k + 0.5)^2 = k^2 + k + 0.25 is
// not, so r is at least 0.25 / (2 r) > 0.005 away from every k + 0.5, again far beyond the float32 slop.
inline int brief_reach(const int8_t* pattern) {
  int r2 = 0;
  for (int k = 0; k < kBriefPoints; ++k) r2 = fast_max(r2, pattern[2 * k] * pattern[2 * k] + pattern[2 * k + 1] * pattern[2 * k + 1]);
  int R = 0;
  while (R * R < r2) ++R;
  return R;
}

// ---- host only

// The default weights: the double kernel exp(-x^2 / (2 sigma^2)) normalised to 1, times 256; the first half rounded tap by tap to
// nearest with the rounding error carried to the next tap, mirrored, the centre tap 256 - 2 * sum.  (7, 2): 18 34 48 56 48 34 18.
inline void brief_gaussian_q8(int ksize, double sigma, uint16_t* out) {
  std::vector<double> k((size_t)ksize);
  double sum = 0;
  for (int i = 0; i < ksize; ++i) { const double x = i - (ksize - 1) / 2; k[i] = std::exp(-x * x / (2 * sigma * sigma)); sum += k[i]; }
  double carry = 0;
  int given = 0;
  for (int i = 0; i < ksize / 2; ++i) {
    const double want = k[i] / sum * 256.0 + carry;
    const int q = (int)std::nearbyint(want);
    carry = want - q;
    out[i] = out[ksize - 1 - i] = (uint16_t)q;
    given += 2 * q;
  }
  out[ksize / 2] = (uint16_t)(256 - given);
}

// B of a whole level (rows `stride` bytes apart) into dst, rows packed
inline void brief_blur_level_host(const uint8_t* src, int rows, int cols, long long stride, const uint16_t* w, uint8_t* dst) {
  std::vector<uint16_t> h((size_t)rows * cols);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) h[(size_t)y * cols + x] = (uint16_t)brief_blur_h(src + y * stride, x, cols, w);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      int acc = 0;
      for (int v = 0; v < kBriefTaps; ++v) acc += (int)w[v] * h[(size_t)brief_reflect101(y + v - kBriefHalo, rows) * cols + x];
      dst[(size_t)y * cols + x] = brief_blur_round(acc);
    }
}

// The 32 bytes of a keypoint on the blurred level (rows `pitch` bytes apart)
inline BriefRot brief_descriptor_host(const uint8_t* blurred, long long pitch, float x, float y, float angle, const int8_t* pattern, uint8_t* desc) {
  const BriefRot r = brief_rotation(angle);
  const uint8_t* centre = blurred + (long long)fast_cv_round(y) * pitch + fast_cv_round(x);
  for (int i = 0; i < 32; ++i) {
    int byte = 0;
    for (int k = 0; k < 8; ++k) byte |= (brief_pair(centre, pitch, r, pattern, 8 * i + k) ? 1 : 0) << k;
    desc[i] = (uint8_t)byte;
  }
  return r;
}

}  // namespace osh
