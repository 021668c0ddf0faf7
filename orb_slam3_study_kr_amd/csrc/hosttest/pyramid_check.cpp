// pyramid_check.cpp -- csrc/orb_pyramid.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make pyramid-check)
// that makes no HIP call and needs no device.  It builds the pyramids of the shapes the tests commit to (tests/pyramid_numpy.py) on
// images and levels allocated at exactly their size, a bordered level at exactly (rows + 2 b) x (cols + 2 b), so that a read or a
// write outside a level or its border is one outside the allocation: the ordinary chain, exact halving in both axes and in one,
// every cols % 4, ratio 1 and upsampling (every clamp), one-row and one-column levels, a 3 x 3 image under a border of 19 (repeated
// reflection, len == 1 after it), borders 0, 3 and 19; with pixels that are constant 0 and 255 (they must stay so), a 0 / 255
// checkerboard and noise.  It checks the table entries against their ranges and the known answers of the reflection.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../orb_pyramid.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static std::vector<uint8_t> make_image(int rows, int cols, int kind) {
  std::vector<uint8_t> img((size_t)rows * cols);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      img[(size_t)y * cols + x] = kind == 0 ? 0 : kind == 1 ? 255 : kind == 2 ? (((x + y) & 1) ? 255 : 0) : (uint8_t)(rng() & 255);
  return img;
}

struct Shape { int rows, cols, n_levels; float inv[4]; int border; };

static long g_levels = 0, g_pixels = 0, g_off_sum = 0;

static int check_tables(int src, int dst, bool rows) {
  std::vector<osh::PyrTap> t((size_t)dst);
  osh::pyr_axis_table(src, dst, rows, t.data());
  for (int d = 0; d < dst; ++d) {
    if (t[d].s0 < 0 || t[d].s0 >= src || t[d].s1 < 0 || t[d].s1 >= src || t[d].s1 < t[d].s0 || t[d].s1 > t[d].s0 + 1) { std::printf("table %d -> %d: entry %d reads %d, %d\n", src, dst, d, t[d].s0, t[d].s1); return 1; }
    if (t[d].w0 < 0 || t[d].w0 > 2048 || t[d].w1 < 0 || t[d].w1 > 2048) { std::printf("table %d -> %d: entry %d has weights %d, %d\n", src, dst, d, t[d].w0, t[d].w1); return 1; }
    if (t[d].w0 + t[d].w1 != 2048) ++g_off_sum;
  }
  return 0;
}

static int check_shape(const Shape& s, int kind) {
  std::vector<uint8_t> prev = make_image(s.rows, s.cols, kind);
  int prows = s.rows, pcols = s.cols;
  for (int l = 0; l < s.n_levels; ++l) {
    const int h = osh::pyr_level_size(s.rows, s.inv[l]), w = osh::pyr_level_size(s.cols, s.inv[l]);
    if (h <= 0 || w <= 0) { std::printf("%dx%d: level %d is empty\n", s.rows, s.cols, l); return 1; }
    if (l == 0 && (h != s.rows || w != s.cols)) { std::printf("%dx%d: level 0 is %dx%d\n", s.rows, s.cols, h, w); return 1; }
    std::vector<uint8_t> cur((size_t)h * w);
    if (l == 0) cur = prev;
    else {
      if (!osh::pyr_is_halving(prows, pcols, h, w) && (check_tables(pcols, w, false) || check_tables(prows, h, true))) return 1;
      osh::pyr_resample_level_host(prev.data(), prows, pcols, pcols, cur.data(), h, w, w);
    }
    if (kind < 2)
      for (uint8_t v : cur) if (v != (kind ? 255 : 0)) { std::printf("%dx%d level %d: a constant image did not stay constant (%d)\n", s.rows, s.cols, l, v); return 1; }
    // the bordered copy at exactly its size
    const int b = s.border, pitch = w + 2 * b;
    std::vector<uint8_t> whole((size_t)(h + 2 * b) * pitch, 0x5a);
    uint8_t* lv = whole.data() + (size_t)b * pitch + b;
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) lv[(long long)y * pitch + x] = cur[(size_t)y * w + x];
    osh::pyr_border_host(lv, h, w, pitch, b);
    if (kind < 2)
      for (uint8_t v : whole) if (v != (kind ? 255 : 0)) { std::printf("%dx%d level %d: the border of a constant level is %d\n", s.rows, s.cols, l, v); return 1; }
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) if (lv[(long long)y * pitch + x] != cur[(size_t)y * w + x]) { std::printf("the border changed the level\n"); return 1; }
    ++g_levels; g_pixels += (long)whole.size();
    prev.swap(cur); prows = h; pcols = w;
  }
  return 0;
}

int main() {
  using osh::pyr_reflect101;
  if (pyr_reflect101(-1, 4) != 1 || pyr_reflect101(-3, 4) != 3 || pyr_reflect101(-4, 4) != 2 || pyr_reflect101(4, 4) != 2 || pyr_reflect101(6, 4) != 0 ||
      pyr_reflect101(7, 4) != 1 || pyr_reflect101(-19, 3) != 1 || pyr_reflect101(21, 3) != 1 || pyr_reflect101(-19, 1) != 0 || pyr_reflect101(5, 1) != 0 ||
      pyr_reflect101(2, 4) != 2 || pyr_reflect101(-2, 2) != 0 || pyr_reflect101(-1, 2) != 1) { std::printf("reflect-101\n"); return 1; }
  if (osh::pyr_level_size(480, 1.f / 1.2f) != 400 || osh::pyr_level_size(5, 0.5f) != 2 || osh::pyr_level_size(7, 0.5f) != 4 || osh::pyr_level_size(40, 0.5f) != 20) { std::printf("level sizes\n"); return 1; }
  // a ratio of 1 copies the level: f = 0 everywhere
  {
    const std::vector<uint8_t> img = make_image(12, 20, 3);
    std::vector<uint8_t> out(img.size());
    osh::pyr_resample_level_host(img.data(), 12, 20, 20, out.data(), 12, 20, 20);
    if (out != img) { std::printf("the ratio 1 changed the level\n"); return 1; }
  }
  const float q = 1.f / 1.2f;
  const Shape shapes[] = {
      {37, 53, 4, {1.f, q, 1.f / 1.44f, 1.f / 1.728f}, 19}, {40, 64, 3, {1.f, .5f, .25f}, 19}, {41, 64, 2, {1.f, .5f}, 19},
      {16, 64, 2, {1.f, q}, 19}, {17, 65, 2, {1.f, q}, 19}, {15, 63, 2, {1.f, q}, 19},
      {30, 40, 2, {1.f, q}, 19}, {30, 41, 2, {1.f, q}, 19}, {30, 42, 2, {1.f, q}, 19}, {30, 43, 2, {1.f, q}, 19},
      {12, 20, 4, {1.f, 1.f, 1.5f, .75f}, 19}, {1, 50, 2, {1.f, .75f}, 19}, {50, 1, 2, {1.f, .75f}, 19}, {2, 50, 2, {1.f, .5f}, 19}, {50, 2, 2, {1.f, .5f}, 19},
      {43, 64, 2, {1.f, .5f}, 19}, {3, 3, 2, {1.f, 1.f / 3.f}, 19},
      {9, 70, 1, {1.f}, 0}, {9, 70, 1, {1.f}, 3}, {9, 70, 1, {1.f}, 19}, {120, 160, 3, {1.f, q, q * q}, 19}};
  for (const Shape& s : shapes) for (int kind = 0; kind < 4; ++kind) if (check_shape(s, kind)) return 1;
  std::printf("pyramid_check: %ld levels, %ld bordered pixels, %ld table entries whose weights do not sum to 2048\n", g_levels, g_pixels, g_off_sum);
  return 0;
}
