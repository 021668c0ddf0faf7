// orb_fast.h -- the integer part of ORBextractor::ComputeKeyPointsOctTree (src/ORBextractor.cc:781-896) restated from the
// definitions: the cell geometry of a pyramid level (:785-822), the FAST-9/16 score of cv::FAST(..., threshold, true) with its 3x3
// strict-maximum test, the two-threshold rule of a cell (:826-869), and IC_Angle (:76-103) with OpenCV's documented scalar
// fastAtan2.  Device code of orb_fast_device.hip; plain C++ as well, so the test library and `make fast-check` run the same
// statements on the host.
//
// Parity rules: the geometry takes the reference's float32 and int steps; scores and moments are integers; the
// polynomial of fastAtan2 is single float32 operations in the written order with contraction off.  One defined skip: a level with
// nCols == 0 or nRows == 0 has no cells (the reference divides by zero there).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OSH_FAST_HD __host__ __device__ inline
#else
#define OSH_FAST_HD inline
#endif

namespace osh {

constexpr int kFastBorder = 16;        // EDGE_THRESHOLD - 3
constexpr int kFastMaxCell = 75;       // wCell < 70, plus the 6 pixels of overlap
constexpr int kFastHalfPatch = 15;     // HALF_PATCH_SIZE
constexpr int kFastMaskWords = (kFastMaxCell * kFastMaxCell + 31) / 32;   // one bit per pixel of a cell's sub-image, row-major

// :785-803 for a level of rows x cols pixels
struct FastGeom {
  int max_x, max_y;     // maxBorderX, maxBorderY
  int n_cols, n_rows;   // 0, 0: the level has no cells
  int w_cell, h_cell;
};
OSH_FAST_HD FastGeom fast_geometry(int rows, int cols) {
  FastGeom g;
  g.max_x = cols - kFastBorder; g.max_y = rows - kFastBorder;
  const float width = (float)(g.max_x - kFastBorder), height = (float)(g.max_y - kFastBorder);
  g.n_cols = (int)(width / 35.f); g.n_rows = (int)(height / 35.f);
  if (g.n_cols <= 0 || g.n_rows <= 0) { g.n_cols = g.n_rows = g.w_cell = g.h_cell = 0; return g; }
  g.w_cell = (int)ceil(width / g.n_cols);
  g.h_cell = (int)ceil(height / g.n_rows);
  return g;
}
// :807-822 for cell (i, j): the sub-image is rows [y0, y0 + h) x columns [x0, x0 + w) of the level.  false: one of the two `continue`s.
struct FastRect { int x0, y0, w, h; };
OSH_FAST_HD bool fast_cell_rect(const FastGeom& g, int i, int j, FastRect& r) {
  const int ini_y = kFastBorder + i * g.h_cell, ini_x = kFastBorder + j * g.w_cell;
  if (ini_y >= g.max_y - 3 || ini_x >= g.max_x - 6) return false;
  const int max_y = ini_y + g.h_cell + 6 > g.max_y ? g.max_y : ini_y + g.h_cell + 6;
  const int max_x = ini_x + g.w_cell + 6 > g.max_x ? g.max_x : ini_x + g.w_cell + 6;
  r.x0 = ini_x; r.y0 = ini_y; r.w = max_x - ini_x; r.h = max_y - ini_y;
  return true;
}
OSH_FAST_HD int fast_cells_of_level(int rows, int cols) {
  const FastGeom g = fast_geometry(rows, cols);
  int n = 0;
  FastRect r;
  for (int i = 0; i < g.n_rows; ++i) for (int j = 0; j < g.n_cols; ++j) n += fast_cell_rect(g, i, j, r) ? 1 : 0;
  return n;
}

OSH_FAST_HD int fast_min(int a, int b) { return a < b ? a : b; }
OSH_FAST_HD int fast_max(int a, int b) { return a > b ? a : b; }

// The score of the pixel at p (rows `pitch` bytes apart; the 16 circle pixels must exist): the largest t at which it is a FAST-9/16
// corner, 0 if there is none.  With d[k] = p_k - v, lo9 / hi9 are the minimum / maximum of d over the 9 circle pixels that start
// at k, built by doubling: windows of 2, of 4, of 8, then the ninth pixel.
template <class Pitch>
OSH_FAST_HD int fast_score_at(const uint8_t* p, Pitch pitch) {
  const int v = p[0];
  int d[16];
  d[0] = p[3 * pitch] - v;        d[1] = p[3 * pitch + 1] - v;   d[2] = p[2 * pitch + 2] - v;   d[3] = p[pitch + 3] - v;
  d[4] = p[3] - v;                d[5] = p[-pitch + 3] - v;      d[6] = p[-2 * pitch + 2] - v;  d[7] = p[-3 * pitch + 1] - v;
  d[8] = p[-3 * pitch] - v;       d[9] = p[-3 * pitch - 1] - v;  d[10] = p[-2 * pitch - 2] - v; d[11] = p[-pitch - 3] - v;
  d[12] = p[-3] - v;              d[13] = p[pitch - 3] - v;      d[14] = p[2 * pitch - 2] - v;  d[15] = p[3 * pitch - 1] - v;
  int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { lo2[k] = fast_min(d[k], d[(k + 1) & 15]); hi2[k] = fast_max(d[k], d[(k + 1) & 15]); }
#pragma unroll
  for (int k = 0; k < 16; ++k) { lo4[k] = fast_min(lo2[k], lo2[(k + 2) & 15]); hi4[k] = fast_max(hi2[k], hi2[(k + 2) & 15]); }
  int best = -256;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int lo9 = fast_min(fast_min(lo4[k], lo4[(k + 4) & 15]), d[(k + 8) & 15]);   // brighter: min of p_k - v over the arc
    const int hi9 = fast_max(fast_max(hi4[k], hi4[(k + 4) & 15]), d[(k + 8) & 15]);   // darker: min of v - p_k = -max of p_k - v
    best = fast_max(best, fast_max(lo9, -hi9));
  }
  return fast_max(best - 1, 0);
}

// Whether the score s at (x, y) of a score map of pitch `pitch` with a one-pixel rim of zeros is a kept corner: positive and
// strictly greater than its eight neighbours.  For s >= t > 0 this does not depend on t.
OSH_FAST_HD bool fast_is_kept(const uint8_t* score, int pitch) {
  const int s = score[0];
  return s > 0 && s > score[-pitch - 1] && s > score[-pitch] && s > score[-pitch + 1] && s > score[-1] && s > score[1] &&
         s > score[pitch - 1] && s > score[pitch] && s > score[pitch + 1];
}

// cvRound: to nearest, halves to even
OSH_FAST_HD int fast_cv_round(float x) { return (int)rintf(x); }

// Half-width of row v of the 31-pixel disc, v = 0 .. 15: the disc of radius 15 made symmetric about its diagonal, as :453-470 leave it
OSH_FAST_HD int fast_disc_half_width(int v) {
  constexpr int half[kFastHalfPatch + 1] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
  return half[v];
}

// The first-order moments of the disc around the pixel at `centre` (rows `pitch` bytes apart), from their definition:
// m10 = sum of u * I(u, v) and m01 = sum of v * I(u, v) over |v| <= 15, |u| <= half width of row |v|.  Integers: any order.
OSH_FAST_HD void fast_ic_moments(const uint8_t* centre, long long pitch, int& m10, int& m01) {
  int sum_u = 0, sum_v = 0;
  for (int v = -kFastHalfPatch; v <= kFastHalfPatch; ++v) {
    const uint8_t* row = centre + v * pitch;
    const int half = fast_disc_half_width(v < 0 ? -v : v);
    int row_total = 0;
#pragma unroll 4
    for (int u = -half; u <= half; ++u) {
      const int I = row[u];
      row_total += I;
      sum_u += u * I;
    }
    sum_v += v * row_total;
  }
  m10 = sum_u; m01 = sum_v;
}

// OpenCV's scalar fastAtan2 (degrees in [0, 360)), every operation a single float32 one
OSH_FAST_HD float fast_atan2(float y, float x) {
#pragma clang fp contract(off)
  const float s = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * s, p3 = -0.3258083974640975f * s, p5 = 0.1555786518463281f * s, p7 = -0.04432655554792128f * s;
  const float eps = (float)DBL_EPSILON;
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + eps);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + eps);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

// ---- host only: a whole level cell by cell, as k_fast_cells and k_fast_emit do it together

enum { kFastAtIni = 0, kFastAtMin = 1, kFastEmpty = 2 };   // used_min_th of a cell

struct FastCorner { float x, y, response; int cell; };

// The kept corners of one cell's sub-image (row-major) under the two-threshold rule; returns kFastAtIni / AtMin / Empty.
inline int fast_cell_host(const uint8_t* level, long long stride, const FastRect& r, int ini_th, int min_th, std::vector<FastCorner>& out,
                          int shift_x, int shift_y, int cell) {
  constexpr int pitch = kFastMaxCell + 2;
  uint8_t score[pitch * pitch] = {0};
  for (int y = 3; y < r.h - 3; ++y)
    for (int x = 3; x < r.w - 3; ++x) {
      const uint8_t* p = level + (long long)(r.y0 + y) * stride + r.x0 + x;
      score[(y + 1) * pitch + x + 1] = (uint8_t)fast_score_at(p, stride);
    }
  int n_ini = 0, n_min = 0;
  for (int y = 3; y < r.h - 3; ++y)
    for (int x = 3; x < r.w - 3; ++x) {
      const uint8_t* s = &score[(y + 1) * pitch + x + 1];
      if (!fast_is_kept(s, pitch)) continue;
      n_ini += s[0] >= ini_th; n_min += s[0] >= min_th;
    }
  const int th = n_ini ? ini_th : min_th;
  if (!n_ini && !n_min) return kFastEmpty;
  for (int y = 3; y < r.h - 3; ++y)
    for (int x = 3; x < r.w - 3; ++x) {
      const uint8_t* s = &score[(y + 1) * pitch + x + 1];
      if (fast_is_kept(s, pitch) && s[0] >= th) out.push_back({(float)(x + shift_x), (float)(y + shift_y), (float)s[0], cell});
    }
  return n_ini ? kFastAtIni : kFastAtMin;
}

// Every cell of a level in (i, j) order: the corners (pt relative to minBorder, :865-866) and one used_min_th entry per cell.
// `cell0` numbers the level's first cell.
inline void fast_level_host(const uint8_t* level, int rows, int cols, long long stride, int ini_th, int min_th, int cell0,
                            std::vector<FastCorner>& out, std::vector<uint8_t>& used_min_th) {
  const FastGeom g = fast_geometry(rows, cols);
  FastRect r;
  for (int i = 0; i < g.n_rows; ++i)
    for (int j = 0; j < g.n_cols; ++j) {
      if (!fast_cell_rect(g, i, j, r)) continue;
      const int cell = cell0 + (int)used_min_th.size();
      used_min_th.push_back((uint8_t)fast_cell_host(level, stride, r, ini_th, min_th, out, j * g.w_cell, i * g.h_cell, cell));
    }
}

// IC_Angle of the keypoint (x, y) of a level; the 31-pixel disc must lie inside the level
inline float fast_ic_angle_host(const uint8_t* level, long long stride, float x, float y, int& m10, int& m01) {
  fast_ic_moments(level + (long long)fast_cv_round(y) * stride + fast_cv_round(x), stride, m10, m01);
  return fast_atan2((float)m01, (float)m10);
}

}  // namespace osh
