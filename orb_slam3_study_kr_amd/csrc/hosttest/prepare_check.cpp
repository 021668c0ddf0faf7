// prepare_check.cpp -- csrc/orb_prepare.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make prepare-check)
// that makes no HIP call and needs no device.  Sources, maps and grey images are heap buffers of exactly their size, so that a read
// outside the source or the maps or a write outside the destination is one outside an allocation: maps whose pixels are set by hand
// to the edges of the definition (sx = -1, the last column and row with a fraction, both rows outside, far outside, products exactly
// on k + 0.5, NaN, the infinities, +-40000, +-32768), on 1, 3 and 4 channels in both orders; an identity map, a half-pixel map, the
// pure colours, a resize through the tables (37 x 53 -> 30 x 41, 12 x 20 -> 18 x 30 upsampling, a 1 x 50 and a 50 x 1 source) and an
// exact halving, on every channel count; a pass-through.  It compares a few known answers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../orb_prepare.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static std::vector<uint8_t> noise(int rows, int cols, int channels) {
  std::vector<uint8_t> img((size_t)rows * cols * channels);
  for (uint8_t& v : img) v = (uint8_t)(rng() & 255);
  return img;
}

static long g_frames = 0, g_pixels = 0;

static osh::PrepSource source(const std::vector<uint8_t>& img, int rows, int cols, int channels, int bgr) {
  return osh::PrepSource{img.data(), (long long)cols * channels, rows, cols, channels, bgr};
}

// The frame into a buffer of exactly its size
static std::vector<uint8_t> run(const osh::PrepSource& S, const std::vector<float>* mx, const std::vector<float>* my, int rows, int cols) {
  std::vector<uint8_t> out((size_t)rows * cols, 0xA7);
  osh::prep_frame_host(S, mx ? mx->data() : nullptr, 4LL * cols, my ? my->data() : nullptr, 4LL * cols, out.data(), rows, cols, cols);
  ++g_frames; g_pixels += (long)rows * cols;
  return out;
}

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // ---- the edges of a remap, on every channel count and order
  const int R = 12, Cc = 20;
  const float edge[][2] = {{-1.f / 32, 3.f}, {19.25f, 2.f}, {4.f, -1.5f}, {100.f, 100.f}, {64.5f / 32, 5.f}, {65.5f / 32, 5.f}, {nan, 5.f}, {inf, 5.f},
                           {40000.f, 5.f}, {5.f, nan}, {-40000.f, 5.f}, {32768.f, 5.f}, {5.f, -inf}, {-32768.f, -32768.f}, {7.f, 11.5f},
                           {-16.5f / 32, 4.f}, {19.f, 11.f}, {-1.f, -1.f}, {19.96875f, 11.96875f}, {5.f, 32769.f}, {3.0e38f, -3.0e38f},
                           {-0.015625f, -0.015625f}, {19.984375f, 11.984375f}, {32767.99f, 0.f}};
  const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
  for (int channels : {1, 3, 4})
    for (int bgr : {0, 1}) {
      const std::vector<uint8_t> img = noise(R, Cc, channels);
      std::vector<float> mx((size_t)R * Cc), my((size_t)R * Cc);
      for (int i = 0; i < R * Cc; ++i) {
        mx[i] = i < n_edge ? edge[i][0] : (float)(rng() % 2400) / 100.f - 2.f;    // -2 .. 22: both sides of the source
        my[i] = i < n_edge ? edge[i][1] : (float)(rng() % 1600) / 100.f - 2.f;
      }
      const std::vector<uint8_t> out = run(source(img, R, Cc, channels, bgr), &mx, &my, R, Cc);
      if (channels == 1) {
        auto s = [&](int r, int c) { return (int)img[(size_t)r * Cc + c]; };
        const int want[] = {(31 * s(3, 0) * 32 + 512) >> 10, (24 * s(2, 19) * 32 + 512) >> 10, 0, 0, s(5, 2), (30 * s(5, 2) + 2 * s(5, 3) + 16) >> 5, 0, 0, 0, 0, 0, 0, 0, 0,
                            (16 * s(11, 7) * 32 + 512) >> 10, (16 * s(4, 0) * 32 + 512) >> 10, s(11, 19), 0, (s(11, 19) + 512) >> 10, 0, 0};
        for (int i = 0; i < (int)(sizeof(want) / sizeof(want[0])); ++i)
          if (out[i] != want[i]) { std::printf("edge %d: %d, not %d\n", i, out[i], want[i]); return 1; }
      }
    }
  // ---- identity and half-pixel maps
  {
    const int r = 9, c = 70;
    const std::vector<uint8_t> img = noise(r, c, 1);
    std::vector<float> mx((size_t)r * c), my((size_t)r * c);
    for (int y = 0; y < r; ++y) for (int x = 0; x < c; ++x) { mx[(size_t)y * c + x] = (float)x; my[(size_t)y * c + x] = (float)y; }
    if (run(source(img, r, c, 1, 0), &mx, &my, r, c) != img) { std::printf("identity map\n"); return 1; }
    for (float& v : mx) v += 0.5f;
    for (float& v : my) v += 0.5f;
    const std::vector<uint8_t> out = run(source(img, r, c, 1, 0), &mx, &my, r, c);
    for (int y = 0; y + 1 < r; ++y)
      for (int x = 0; x + 1 < c; ++x) {
        const int want = (img[(size_t)y * c + x] + img[(size_t)y * c + x + 1] + img[(size_t)(y + 1) * c + x] + img[(size_t)(y + 1) * c + x + 1] + 2) >> 2;
        if (out[(size_t)y * c + x] != want) { std::printf("half-pixel map at %d, %d\n", y, x); return 1; }
      }
  }
  // ---- grey: the pure colours in both orders, with and without a fourth channel
  for (int channels : {3, 4})
    for (int bgr : {0, 1}) {
      std::vector<uint8_t> img = noise(1, 4, channels);
      const uint8_t rgb[4][3] = {{255, 0, 0}, {0, 255, 0}, {0, 0, 255}, {255, 255, 255}};
      for (int i = 0; i < 4; ++i) for (int ch = 0; ch < 3; ++ch) img[(size_t)i * channels + (bgr ? 2 - ch : ch)] = rgb[i][ch];
      const std::vector<uint8_t> out = run(source(img, 1, 4, channels, bgr), nullptr, nullptr, 1, 4);
      if (out[0] != 76 || out[1] != 150 || out[2] != 29 || out[3] != 255) { std::printf("grey of the pure colours: %d %d %d %d\n", out[0], out[1], out[2], out[3]); return 1; }
    }
  // ---- resize through the tables, exact halving, pass-through
  const int shapes[][4] = {{37, 53, 30, 41}, {12, 20, 18, 30}, {1, 50, 1, 38}, {50, 1, 38, 1}, {40, 64, 20, 32}, {2, 2, 1, 1}, {1, 50, 1, 50}, {7, 5, 7, 5}, {3, 3, 1, 1}};
  for (const auto& s : shapes)
    for (int channels : {1, 3, 4}) {
      const std::vector<uint8_t> img = noise(s[0], s[1], channels);
      const std::vector<uint8_t> out = run(source(img, s[0], s[1], channels, channels == 4), nullptr, nullptr, s[2], s[3]);
      if (channels == 1 && s[0] == s[2] && s[1] == s[3] && out != img) { std::printf("pass-through\n"); return 1; }
      if (channels == 1 && osh::pyr_is_halving(s[0], s[1], s[2], s[3])) {
        std::vector<uint8_t> want((size_t)s[2] * s[3]);
        osh::pyr_resample_level_host(img.data(), s[0], s[1], s[1], want.data(), s[2], s[3], s[3]);
        if (out != want) { std::printf("halving\n"); return 1; }
      }
      if (channels == 1 && osh::prep_mode(s[0], s[1], s[2], s[3]) == osh::kPrepResize) {   // one channel: the pyramid's own level
        std::vector<uint8_t> want((size_t)s[2] * s[3]);
        osh::pyr_resample_level_host(img.data(), s[0], s[1], s[1], want.data(), s[2], s[3], s[3]);
        if (out != want) { std::printf("resize %d x %d -> %d x %d\n", s[0], s[1], s[2], s[3]); return 1; }
      }
    }
  if (osh::prep_usable(nan) || osh::prep_usable(inf) || osh::prep_usable(-inf) || osh::prep_usable(32768.5f) || !osh::prep_usable(32768.f) || !osh::prep_usable(-32768.f)) { std::printf("usable\n"); return 1; }
  if (osh::prep_q5(2.015625f) != 64 || osh::prep_q5(2.046875f) != 66 || osh::prep_q5(-0.515625f) != -16 || osh::prep_q5(-32768.f) != -1048576) { std::printf("q5\n"); return 1; }
  std::printf("prepare_check: %ld frames, %ld pixels\n", g_frames, g_pixels);
  return 0;
}
