// extractor_host_check.cpp -- the steps of csrc/host/orb_extract_steps.h (what the bodies of csrc/host/ORBextractor.cc share and
// that makes no device call) on plain host memory, for a run under a sanitizer: the write-back on exactly-sized arrays against a plain
// restatement of reference src/ORBextractor.cc:1120-1167, the level shapes against known answers, the sampling table with its fit
// flag.  A program of its own (`make extractor-host-check`), in no library; it makes no HIP call and needs no device.
#include <cstdio>
#include <vector>

#include "../host/orb_extract_steps.h"

using namespace ORB_SLAM3;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Point2f { float x, y; Point2f& operator*=(float s) { x *= s; y *= s; return *this; } };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
struct Point { int x, y; };

static const float kScale[3] = {1.f, 1.5f, 2.f};
static const int kLapping[2] = {100, 200};

// One keypoint at (x, 7) of `level`; the other fields tell the keypoints apart
static KeyPoint at(float x, int level, int id) { return {{x, 7.f}, 31.f * kScale[level], 10.f * id, 0.5f + id, level, -1}; }

// The write-back as the reference's loops state it, on vectors; then WriteBack into arrays of exactly n keypoints and n * 32 bytes
static void check_write_back(const char* what, const std::vector<KeyPoint>& in, int expected_mono) {
  const int n = (int)in.size();
  std::vector<uint8_t> desc((size_t)n * 32);
  for (size_t i = 0; i < desc.size(); ++i) desc[i] = (uint8_t)(i * 7 + 3);
  std::vector<KeyPoint> exp(n);
  std::vector<uint8_t> exp_desc((size_t)n * 32);
  int monoIndex = 0, stereoIndex = n - 1;
  for (int i = 0; i < n; ++i) {
    KeyPoint kp = in[i];
    if (kp.octave != 0) { kp.pt.x *= kScale[kp.octave]; kp.pt.y *= kScale[kp.octave]; }
    int where;
    if (kp.pt.x >= kLapping[0] && kp.pt.x <= kLapping[1]) { where = stereoIndex; stereoIndex--; }
    else { where = monoIndex; monoIndex++; }
    exp[where] = kp;
    for (int b = 0; b < 32; ++b) exp_desc[32 * (size_t)where + b] = desc[32 * (size_t)i + b];
  }
  std::vector<KeyPoint> got(n);
  std::vector<uint8_t> got_desc((size_t)n * 32);
  WriteBack<KeyPoint> place(n, kScale, kLapping, got.data(), got_desc.data(), 32);
  for (int i = 0; i < n; ++i) place(in[i], desc.data() + 32 * (size_t)i);
  const int mono = place.monoIndex;
  bool same = mono == monoIndex && mono == expected_mono && got_desc == exp_desc;
  for (int i = 0; i < n && same; ++i)
    same = got[i].pt.x == exp[i].pt.x && got[i].pt.y == exp[i].pt.y && got[i].size == exp[i].size && got[i].angle == exp[i].angle &&
           got[i].response == exp[i].response && got[i].octave == exp[i].octave && got[i].class_id == exp[i].class_id;
  if (!same) { std::printf("write-back, %s: differs from the restatement (monoIndex %d, expected %d)\n", what, mono, expected_mono); ++failures; }
}

// mvInvScaleFactor as the stand-in constructor (and the reference's) fills it
static std::vector<float> inv_scale(int nlevels, float scaleFactor) {
  std::vector<float> scale(nlevels), inv(nlevels);
  for (int i = 0; i < nlevels; ++i) {
    scale[i] = i ? (float)(scale[i - 1] * (double)scaleFactor) : 1.0f;
    inv[i] = 1.0f / scale[i];
  }
  return inv;
}

// The first level LevelShape refuses (nlevels: none); the shapes before it must be the known ones
static int check_shapes(int rows, int cols, int nlevels, const int (*expected)[2]) {
  const std::vector<float> inv = inv_scale(nlevels, 1.2f);
  for (int l = 0; l < nlevels; ++l) {
    int h = -1, w = -1;
    if (!LevelShape(rows, cols, inv[l], h, w)) return l;
    CHECK(h == expected[l][0] && w == expected[l][1]);
  }
  return nlevels;
}

int main() {
  check_write_back("no keypoint", {}, 0);
  check_write_back("one keypoint outside", {at(5.f, 0, 1)}, 1);
  check_write_back("one keypoint inside", {at(150.f, 0, 1)}, 0);
  check_write_back("all inside", {at(100.5f, 0, 1), at(150.f, 0, 2), at(80.f, 1, 3), at(99.f, 2, 4)}, 0);
  check_write_back("none inside", {at(99.5f, 0, 1), at(200.5f, 0, 2), at(10.f, 1, 3), at(101.f, 2, 4)}, 4);
  // on the bounds (inside), at level 0 and after the scaling (50 * 2 = 100, 100 * 2 = 200), and the nearest floats beyond them
  check_write_back("on the bounds", {at(100.f, 0, 1), at(200.f, 0, 2), at(50.f, 2, 3), at(100.f, 2, 4)}, 0);
  check_write_back("beside the bounds", {at(std::nextafter(100.f, 0.f), 0, 1), at(std::nextafter(200.f, 300.f), 0, 2), at(std::nextafter(50.f, 0.f), 2, 3)}, 3);
  check_write_back("levels mixed", {at(150.f, 0, 1), at(20.f, 0, 2), at(100.f, 1, 3), at(10.f, 1, 4), at(75.f, 2, 5), at(150.f, 2, 6), at(199.f, 0, 7)}, 3);

  static const int k752[8][2] = {{480, 752}, {400, 627}, {333, 522}, {278, 435}, {231, 363}, {193, 302}, {161, 252}, {134, 210}};
  static const int k67[4][2] = {{67, 67}, {56, 56}, {47, 47}, {39, 39}};
  static const int k40[4][2] = {{40, 1}, {33, 1}, {28, 1}, {23, 1}};
  CHECK(check_shapes(480, 752, 8, k752) == 8);
  CHECK(check_shapes(67, 67, 4, k67) == 4);
  CHECK(check_shapes(40, 1, 8, k40) == 4);   // 40 rows by 1 column: nearbyint(1 * 0.48225) = 0 at level 4
  int h, w;
  CHECK(!LevelShape(480, 752, 1500.f, h, w) && w == 0 && h == 720000);   // 752 * 1500 is beyond the guard
  CHECK(!LevelShape(480, 752, -1.f, h, w) && h == 0 && w == 0);
  CHECK(kEdge == 19);

  // the stand-in constructor's table (csrc/hosttest/orbextractor.cc): 512 points in [-13, 12]^2 from a fixed generator
  std::vector<Point> pattern(512);
  uint32_t state = 0x0b5e55edu;
  for (Point& p : pattern) {
    state = state * 1664525u + 1013904223u; p.x = (int)((state >> 8) % 26u) - 13;
    state = state * 1664525u + 1013904223u; p.y = (int)((state >> 8) % 26u) - 13;
  }
  pattern[0] = {-13, -13};
  std::vector<int8_t> table(1024);
  CHECK(PatternTable(pattern.data(), table.data()));
  for (int i = 0; i < 512; ++i) CHECK(table[2 * i] == pattern[i].x && table[2 * i + 1] == pattern[i].y);
  pattern[17] = {127, -128};
  CHECK(PatternTable(pattern.data(), table.data()) && table[34] == 127 && table[35] == -128);
  pattern[511].y = 128;
  CHECK(!PatternTable(pattern.data(), table.data()));
  pattern[511].y = 0; pattern[0].x = -129;
  CHECK(!PatternTable(pattern.data(), table.data()));

  if (failures) { std::printf("extractor_host_check: %d failure(s)\n", failures); return 1; }
  std::printf("extractor_host_check ok\n");
  return 0;
}
