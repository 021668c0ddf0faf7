// fast_check.cpp -- csrc/orb_fast.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make fast-check) that makes
// no HIP call and needs no device.  It runs the cell geometry, the FAST score with its strict-maximum test, the two-threshold rule
// and IC_Angle on images allocated at exactly their size (a read outside a level is a read outside the allocation): the smallest
// level with a cell, levels with a clipped and a removed last cell in either direction, a 160 x 120 level, with pixels that are
// constant, a 0 / 255 checkerboard (the largest differences), isolated dots and noise, at the lowest and highest thresholds, and
// the keypoints whose 31-pixel disc touches the corners of its level.  It checks that every corner lies where its cell has scores,
// that responses respect the threshold the cell was decided at, and the known answers of fastAtan2.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../orb_fast.h"

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int check_level(int rows, int cols, int kind, int ini_th, int min_th, long& corners) {
  std::vector<uint8_t> img((size_t)rows * cols);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      uint8_t v = 0;
      switch (kind) {
        case 0: v = 113; break;
        case 1: v = ((x + y) & 1) ? 255 : 0; break;
        case 2: v = (x % 9 == 4 && y % 9 == 4) ? (uint8_t)(40 + (x * 7 + y * 13) % 200) : 30; break;
        default: v = (uint8_t)(100 + rng() % 56); break;
      }
      img[(size_t)y * cols + x] = v;
    }
  const osh::FastGeom g = osh::fast_geometry(rows, cols);
  std::vector<osh::FastCorner> out;
  std::vector<uint8_t> used;
  osh::fast_level_host(img.data(), rows, cols, cols, ini_th, min_th, 0, out, used);
  if ((int)used.size() != osh::fast_cells_of_level(rows, cols)) { std::printf("%dx%d: %zu cells, %d expected\n", rows, cols, used.size(), osh::fast_cells_of_level(rows, cols)); return 1; }
  // the cell rectangles again, to place every corner
  std::vector<osh::FastRect> rects;
  std::vector<int> sx, sy;
  osh::FastRect r;
  for (int i = 0; i < g.n_rows; ++i) for (int j = 0; j < g.n_cols; ++j) if (osh::fast_cell_rect(g, i, j, r)) { rects.push_back(r); sx.push_back(j * g.w_cell); sy.push_back(i * g.h_cell); }
  for (const osh::FastRect& q : rects)
    if (q.x0 < osh::kFastBorder || q.y0 < osh::kFastBorder || q.x0 + q.w > cols - osh::kFastBorder || q.y0 + q.h > rows - osh::kFastBorder || q.w > osh::kFastMaxCell ||
        q.h > osh::kFastMaxCell || q.w < 7 || q.h < 4) { std::printf("%dx%d: cell %d %d %d %d\n", rows, cols, q.x0, q.y0, q.w, q.h); return 1; }
  int last_cell = -1;
  for (const osh::FastCorner& c : out) {
    if (c.cell < last_cell || c.cell >= (int)rects.size()) { std::printf("%dx%d: cells out of order\n", rows, cols); return 1; }
    last_cell = c.cell;
    const osh::FastRect& q = rects[c.cell];
    const int x = (int)c.x - sx[c.cell], y = (int)c.y - sy[c.cell];
    const int th = used[c.cell] == osh::kFastAtIni ? ini_th : min_th;
    if (x < 3 || x >= q.w - 3 || y < 3 || y >= q.h - 3 || c.response < (float)th || c.response > 254.f || used[c.cell] == osh::kFastEmpty) {
      std::printf("%dx%d kind %d: corner (%g, %g) response %g of cell %d\n", rows, cols, kind, c.x, c.y, c.response, c.cell); return 1;
    }
  }
  if (kind == 0 && !out.empty()) { std::printf("%dx%d: corners on a constant image\n", rows, cols); return 1; }
  corners += (long)out.size();
  // IC_Angle where the disc touches the level's corners, and at halves that round to them
  const float xs[] = {15.f, 15.5f, 14.5001f, (float)(cols - 16), (float)(cols - 16) - 0.5f}, ys[] = {15.f, (float)(rows - 16), (float)(rows - 16) + 0.49f};
  for (float x : xs) for (float y : ys) {
    if (osh::fast_cv_round(x) < 15 || osh::fast_cv_round(x) > cols - 16 || osh::fast_cv_round(y) < 15 || osh::fast_cv_round(y) > rows - 16) continue;
    int m10, m01;
    const float a = osh::fast_ic_angle_host(img.data(), cols, x, y, m10, m01);
    if (!(a >= 0.f && a <= 360.f)) { std::printf("%dx%d: angle %g\n", rows, cols, a); return 1; }
    if (kind == 0 && (m10 || m01 || a != 0.f)) { std::printf("%dx%d: moments of a constant image\n", rows, cols); return 1; }
  }
  return 0;
}

int main() {
  if (osh::fast_atan2(0.f, 1.f) != 0.f || osh::fast_atan2(1.f, 0.f) != 90.f || osh::fast_atan2(0.f, -1.f) != 180.f || osh::fast_atan2(-1.f, 0.f) != 270.f ||
      osh::fast_atan2(0.f, 0.f) != 0.f) { std::printf("fastAtan2 on the axes\n"); return 1; }
  if (osh::fast_cv_round(14.5f) != 14 || osh::fast_cv_round(15.5f) != 16 || osh::fast_cv_round(-0.5f) != 0) { std::printf("cvRound\n"); return 1; }
  const int shapes[][2] = {{67, 67}, {67, 66}, {66, 67}, {70, 73}, {67, 2133}, {2133, 67}, {120, 160}, {101, 136}};
  const int ths[][2] = {{20, 7}, {1, 1}, {255, 255}, {255, 1}};
  long corners = 0, levels = 0;
  for (const auto& s : shapes) for (int kind = 0; kind < 4; ++kind) for (const auto& t : ths) {
    if (check_level(s[0], s[1], kind, t[0], t[1], corners)) return 1;
    ++levels;
  }
  std::printf("fast_check: %ld levels, %ld corners\n", levels, corners);
  return 0;
}
