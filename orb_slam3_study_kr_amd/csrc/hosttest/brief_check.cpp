// brief_check.cpp -- csrc/orb_brief.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make brief-check) that
// makes no HIP call and needs no device.  It runs the blur and the descriptor on images allocated at exactly their size (a read
// outside a level is a read outside the allocation): the smallest level the blur takes (4 x 4), the smallest level that holds a
// keypoint for a table of reach 19 (39 x 39), odd sizes, with pixels that are constant 0 and 255 (they blur to themselves), a
// 0 / 255 checkerboard and noise; keypoints at exactly R pixels from every edge, at halves that round onto that limit, at the
// angles that turn the table's farthest point onto each edge, and tables of the extreme reaches 0 and 22.  It checks the default
// weights, that a rounded offset never exceeds the reach at any of 3600 angles, and the known answers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../orb_brief.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static std::vector<uint8_t> make_level(int rows, int cols, int kind) {
  std::vector<uint8_t> img((size_t)rows * cols);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      img[(size_t)y * cols + x] = kind == 0 ? 0 : kind == 1 ? 255 : kind == 2 ? (((x + y) & 1) ? 255 : 0) : (uint8_t)(rng() & 255);
  return img;
}

static void make_table(int8_t* t, int lo, int hi, int fx, int fy) {
  for (int k = 0; k < osh::kBriefPoints; ++k) { t[2 * k] = (int8_t)(lo + (int)(rng() % (unsigned)(hi - lo + 1))); t[2 * k + 1] = (int8_t)(lo + (int)(rng() % (unsigned)(hi - lo + 1))); }
  t[0] = (int8_t)fx; t[1] = (int8_t)fy;   // the farthest point
}

static int check_level(int rows, int cols, int kind, const uint16_t* w, const int8_t* table, long& descriptors) {
  const std::vector<uint8_t> img = make_level(rows, cols, kind);
  std::vector<uint8_t> blurred((size_t)rows * cols);
  osh::brief_blur_level_host(img.data(), rows, cols, cols, w, blurred.data());
  if (kind < 2)
    for (uint8_t v : blurred) if (v != (kind ? 255 : 0)) { std::printf("%dx%d: a constant level does not blur to itself\n", rows, cols); return 1; }
  const int R = osh::brief_reach(table);
  if (rows < 2 * R + 1 || cols < 2 * R + 1) return 0;
  const float xs[] = {(float)R, (float)R + 0.5f, (float)R - 0.5f, (float)(cols - 1 - R), (float)(cols - 1 - R) + 0.5f, (float)(cols - 1 - R) - 0.5f};
  const float ys[] = {(float)R, (float)R + 0.5f, (float)R - 0.5f, (float)(rows - 1 - R), (float)(rows - 1 - R) + 0.5f, (float)(rows - 1 - R) - 0.5f};
  const float base = (float)(std::atan2((double)table[1], (double)table[0]) * 180.0 / 3.14159265358979323846);
  const float angles[] = {0.f, 90.f, 180.f, 270.f, 30.f, 60.f, 359.99f, -base, 90.f - base, 180.f - base, 270.f - base, 45.f, 123.456f};
  for (float x : xs) for (float y : ys) {
    const int cx = osh::fast_cv_round(x), cy = osh::fast_cv_round(y);
    if (cx - R < 0 || cx + R >= cols || cy - R < 0 || cy + R >= rows) continue;
    for (float a : angles) {
      uint8_t desc[32];
      osh::brief_descriptor_host(blurred.data(), cols, x, y, a, table, desc);
      if (kind < 2) for (uint8_t d : desc) if (d) { std::printf("%dx%d: a bit set on a constant level\n", rows, cols); return 1; }
      ++descriptors;
    }
  }
  return 0;
}

int main() {
  uint16_t w[7];
  osh::brief_gaussian_q8(7, 2.0, w);
  const uint16_t expect[7] = {18, 34, 48, 56, 48, 34, 18};
  for (int k = 0; k < 7; ++k) if (w[k] != expect[k]) { std::printf("default weight %d is %d\n", k, w[k]); return 1; }
  if (osh::brief_reflect101(-3, 4) != 3 || osh::brief_reflect101(6, 4) != 0 || osh::brief_reflect101(4, 4) != 2 || osh::brief_reflect101(2, 4) != 2) { std::printf("reflect-101\n"); return 1; }
  const osh::BriefRot r30 = osh::brief_rotation(30.f), r0 = osh::brief_rotation(0.f);
  if (r30.b != 0.5f || r0.a != 1.f || r0.b != 0.f) { std::printf("rotation: sin 30 = %.9g\n", r30.b); return 1; }
  int dx, dy;
  osh::brief_offset(r30, 5, 0, dx, dy);   // 2.5 -> 2
  if (dy != 2) { std::printf("offset 2.5 went to %d\n", dy); return 1; }
  osh::brief_offset(r30, 7, 0, dx, dy);   // 3.5 -> 4
  if (dy != 4) { std::printf("offset 3.5 went to %d\n", dy); return 1; }

  int8_t tables[4][2 * osh::kBriefPoints];
  make_table(tables[0], -13, 12, -13, -13);   // the reach of the usual table: 19
  make_table(tables[1], -15, 15, 15, -15);    // the largest the entry takes: 22
  make_table(tables[2], 0, 0, 0, 0);          // 0
  make_table(tables[3], -13, 12, 0, 13);      // an axis point of radius 13 among shorter ones
  for (int k = 0; k < osh::kBriefPoints; ++k) if (k) { tables[3][2 * k] = (int8_t)(tables[3][2 * k] / 2); tables[3][2 * k + 1] = (int8_t)(tables[3][2 * k + 1] / 2); }
  const int reaches[4] = {19, 22, 0, 13};
  for (int t = 0; t < 4; ++t) {
    if (osh::brief_reach(tables[t]) != reaches[t]) { std::printf("reach of table %d is %d\n", t, osh::brief_reach(tables[t])); return 1; }
    for (int step = 0; step < 3600; ++step) {
      const osh::BriefRot r = osh::brief_rotation((float)step * 0.1f);
      for (int k = 0; k < osh::kBriefPoints; ++k) {
        osh::brief_offset(r, tables[t][2 * k], tables[t][2 * k + 1], dx, dy);
        if (dx < -reaches[t] || dx > reaches[t] || dy < -reaches[t] || dy > reaches[t]) { std::printf("table %d: offset (%d, %d) beyond %d\n", t, dx, dy, reaches[t]); return 1; }
      }
    }
  }
  const uint16_t identity[7] = {0, 0, 0, 256, 0, 0, 0}, skew[7] = {256, 0, 0, 0, 0, 0, 0}, lopsided[7] = {1, 2, 3, 4, 5, 6, 235};
  const uint16_t* weights[] = {w, identity, skew, lopsided};
  const int shapes[][2] = {{4, 4}, {4, 50}, {50, 4}, {39, 39}, {45, 52}, {39, 40}, {40, 39}, {45, 45}, {17, 65}, {64, 16}, {90, 120}};
  long levels = 0, descriptors = 0;
  for (const auto& s : shapes) for (int kind = 0; kind < 4; ++kind) for (const uint16_t* wk : weights) for (int t = 0; t < 4; ++t) {
    if (check_level(s[0], s[1], kind, wk, tables[t], descriptors)) return 1;
    ++levels;
  }
  // the identity weights return the level
  const std::vector<uint8_t> img = make_level(23, 31, 3);
  std::vector<uint8_t> out(img.size());
  osh::brief_blur_level_host(img.data(), 23, 31, 31, identity, out.data());
  if (out != img) { std::printf("the identity weights changed the level\n"); return 1; }
  std::printf("brief_check: %ld levels, %ld descriptors\n", levels, descriptors);
  return 0;
}
