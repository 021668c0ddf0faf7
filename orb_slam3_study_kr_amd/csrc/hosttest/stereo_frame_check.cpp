// stereo_frame_check.cpp -- the host half of the rectified stereo matcher (csrc/stereo_frame.h) on plain host memory, for a run under a
// sanitizer: the validator on exactly-sized keypoint arrays for both kinds of frame, the token checks against a PyramidTable through
// commit and invalidate, and the level plans (brought: the used levels packed into an arena of exactly img_bytes; resident: the sizes
// and offsets of the table).  A program of its own (`make stereo-frame-check`), in no library; it makes no HIP call and needs no device.
#include <cstdio>
#include <string>
#include <vector>

#include "../stereo_frame.h"

namespace osh {
static char last_error[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(last_error, sizeof last_error, fmt, ap);
  va_end(ap);
}
}  // namespace osh
using namespace osh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, last_error); ++failures; } } while (0)
static bool said(const char* what) { return std::strstr(last_error, what) != nullptr; }

// Keypoints of their own allocations, exactly as long as the counts say
struct Keypoints {
  std::vector<float> lxy, rxy;
  std::vector<int32_t> loct, roct;
  std::vector<uint8_t> ldesc, rdesc;
  std::vector<float> ur, depth;
  float sf[3] = {1.f, 1.2f, 1.44f}, isf[3] = {1.f, 1.f / 1.2f, 1.f / 1.44f};
  Keypoints(int nl, int nr) : lxy(2 * nl, 20.f), rxy(2 * nr, 18.f), loct(nl, 0), roct(nr, 0), ldesc(32 * nl, 1), rdesc(32 * nr, 2), ur(nl), depth(nl) {
    for (int i = 0; i < nl; ++i) loct[i] = i % 2 ? 2 : 0;   // level 1 is named by no left keypoint
    for (int i = 0; i < nr; ++i) roct[i] = i % 3;
  }
  template <class Frame>
  Frame frame() const {
    Frame f{};
    f.n_left = (int)loct.size(); f.n_right = (int)roct.size();
    f.left_xy = lxy.data(); f.left_octave = loct.data(); f.left_desc = ldesc.data();
    f.right_xy = rxy.data(); f.right_octave = roct.data(); f.right_desc = rdesc.data();
    f.n_levels = 3; f.scale_factors = sf; f.inv_scale_factors = isf; f.bf = 40.f; f.b = 1.f;
    return f;
  }
  osh_stereo_result result() { return {ur.data(), depth.data(), nullptr, nullptr, nullptr, nullptr, nullptr}; }
};

// What both kinds of frame are refused for alike
template <class Levels, class Frame>
static void check_validation(Frame base, Keypoints& kp) {
  const osh_stereo_result r = kp.result();
  const auto rc = [&](const Frame& f) { return stereo_validate_frame<Levels>(7, f, r, 0x3FFFFFu); };
  CHECK(rc(base) == OSH_OK);
  Frame f = base;
  f.n_left = -1; CHECK(rc(f) == OSH_ERR_INVALID && said("frame 7: negative keypoint count"));
  f = base; f.n_levels = 0; CHECK(rc(f) == OSH_ERR_INVALID && said("n_levels 0 outside"));
  f = base; f.n_levels = OSH_STEREO_MAX_LEVELS + 1; CHECK(rc(f) == OSH_ERR_INVALID && said("outside [1, 16]"));
  f = base; f.n_right = 0x400000; CHECK(rc(f) == OSH_ERR_UNSUPPORTED && said("n_right exceeds"));
  f = base; f.inv_scale_factors = nullptr; CHECK(rc(f) == OSH_ERR_INVALID && said("NULL scale factors or pyramid"));
  f = base; f.left_desc = nullptr; CHECK(rc(f) == OSH_ERR_INVALID && said("NULL left keypoint or result array"));
  f = base; f.right_octave = nullptr; CHECK(rc(f) == OSH_ERR_INVALID && said("NULL right keypoint array"));
  const osh_stereo_result no_depth{kp.ur.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  CHECK(stereo_validate_frame<Levels>(7, base, no_depth, 0x3FFFFFu) == OSH_ERR_INVALID && said("NULL left keypoint or result array"));
  const float bad_b[4] = {0.f, -1.f, NAN, INFINITY};
  for (float b : bad_b) { f = base; f.b = b; CHECK(rc(f) == OSH_ERR_INVALID && said("bad bf / b")); }
  f = base; f.bf = NAN; CHECK(rc(f) == OSH_ERR_INVALID && said("bad bf / b"));
  kp.lxy.back() = NAN; CHECK(rc(base) == OSH_ERR_INVALID && said("keypoint coordinate not finite")); kp.lxy.back() = 20.f;
  kp.rxy.front() = -2.0e6f; CHECK(rc(base) == OSH_ERR_INVALID && said("keypoint coordinate not finite")); kp.rxy.front() = 18.f;
  kp.roct.back() = 3; CHECK(rc(base) == OSH_ERR_INVALID && said("right octave 3 outside [0, 3)")); kp.roct.back() = 0;
  kp.loct.back() = -1; CHECK(rc(base) == OSH_ERR_INVALID && said("left octave -1 outside [0, 3)")); kp.loct.back() = 0;
  // an empty side may hand over NULL arrays
  f = base; f.n_left = 0; f.left_xy = nullptr; f.left_octave = nullptr; f.left_desc = nullptr;
  const osh_stereo_result none{};
  CHECK(stereo_validate_frame<Levels>(7, f, none, 0x3FFFFFu) == OSH_OK);
  f = base; f.n_right = 0; f.right_xy = nullptr; f.right_octave = nullptr; f.right_desc = nullptr;
  CHECK(rc(f) == OSH_OK);
}

// A level of its own allocation, exactly as long as its last row needs
struct Image {
  int rows, cols, stride;
  std::vector<unsigned char> data;
  Image(int rows_, int cols_, int stride_, int seed) : rows(rows_), cols(cols_), stride(stride_), data((size_t)(rows_ - 1) * stride_ + cols_) {
    for (size_t i = 0; i < data.size(); ++i) data[i] = (unsigned char)(seed + 5 * i);
  }
  osh_stereo_image view() const { return {data.data(), rows, cols, stride}; }
};

static void check_brought() {
  Keypoints kp(5, 4);
  const Image l0(9, 12, 15, 1), l2(6, 8, 8, 2), r0(9, 11, 11, 3), r2(6, 7, 9, 4);
  const osh_stereo_image none{nullptr, 0, 0, 0};
  const osh_stereo_image left[3] = {l0.view(), none, l2.view()}, right[3] = {r0.view(), none, r2.view()};   // level 1 is not used: it may be NULL
  osh_stereo_frame f = kp.frame<osh_stereo_frame>();
  f.left_pyramid = left; f.right_pyramid = right;
  check_validation<BroughtStereoLevels>(f, kp);
  const osh_stereo_result r = kp.result();
  osh_stereo_frame g = f;
  g.right_pyramid = nullptr; CHECK(stereo_validate_frame<BroughtStereoLevels>(0, g, r, 0x3FFFFFu) == OSH_ERR_INVALID && said("NULL scale factors or pyramid"));
  const osh_stereo_image broken[3] = {r0.view(), none, none};
  g = f; g.right_pyramid = broken;
  CHECK(stereo_validate_frame<BroughtStereoLevels>(0, g, r, 0x3FFFFFu) == OSH_ERR_INVALID && said("level 2 (right) is used by a left keypoint"));
  const osh_stereo_image narrow[3] = {{l0.data.data(), 9, 12, 11}, none, l2.view()};
  g = f; g.left_pyramid = narrow;
  CHECK(stereo_validate_frame<BroughtStereoLevels>(0, g, r, 0x3FFFFFu) == OSH_ERR_INVALID && said("level 0 (left) is used by a left keypoint"));
  const osh_stereo_image flat[3] = {{l0.data.data(), 0, 12, 15}, none, l2.view()};
  g = f; g.left_pyramid = flat;
  CHECK(stereo_validate_frame<BroughtStereoLevels>(0, g, r, 0x3FFFFFu) == OSH_ERR_INVALID && said("left_pyramid[0].rows must be positive"));

  // the plan: levels 0 and 2 of both sides, left before right, packed into an arena of exactly img_bytes
  StereoFrameDev d = stereo_frame_dev(f.n_left, f.n_right, 10, 20, f.n_levels, f.bf, f.b, f.scale_factors, f.inv_scale_factors);
  size_t img_bytes = 64;   // the frame before this one took 64 bytes
  stereo_plan_brought(f, d, img_bytes);
  CHECK(d.n_left == 5 && d.n_right == 4 && d.left_base == 10 && d.right_base == 20 && d.n_rows == 9 && d.n_levels == 3);
  CHECK(d.sf[2] == 1.44f && d.isf[1] == 1.f / 1.2f && d.sf[3] == 1.f && d.isf[15] == 1.f);
  CHECK(d.off_l[0] == 64 && d.off_r[0] == 64 + 108 && d.off_l[1] == -1 && d.off_r[1] == -1);
  CHECK(d.off_l[2] == 64 + 108 + 99 && d.off_r[2] == 64 + 108 + 99 + 48 && img_bytes == 64 + 108 + 99 + 48 + 42);
  CHECK(d.rows_l[2] == 6 && d.cols_l[2] == 8 && d.rows_r[2] == 6 && d.cols_r[2] == 7 && d.rows_l[1] == 0 && d.off_l[3] == -1);
  std::vector<unsigned char> arena(img_bytes, 0);
  for (int l = 0; l < 3; ++l) {
    if (d.off_l[l] < 0) continue;
    pack_level(arena.data() + d.off_l[l], left[l]);
    pack_level(arena.data() + d.off_r[l], right[l]);
  }
  CHECK(arena[d.off_l[0] + 12] == l0.data[15] && arena[d.off_r[2] + 7 * 5 + 6] == r2.data[9 * 5 + 6] && arena[img_bytes - 1] == r2.data.back());
}

// The resident table as a build of two pairs lays it out: the level 0 of the four frames first, then the other levels frame after
// frame; the last frame has two levels only
static uint64_t commit_resident(PyramidTable& t) {
  const int n_levels[4] = {3, 3, 3, 2};
  const int rows[3] = {10, 8, 7}, cols[3] = {12, 10, 8};
  std::vector<FastFrameHost> fh;
  std::vector<FastLevelHost> lh;
  long long bytes = 0;
  for (int k = 0; k < 4; ++k) {
    fh.push_back({(int)lh.size(), n_levels[k], 0, 0});
    for (int l = 0; l < n_levels[k]; ++l) lh.push_back({0, rows[l], cols[l] + k, 0, 0});
    lh[fh[k].level0].img_off = bytes;
    bytes += rows[0] * (cols[0] + k);
  }
  for (int k = 0; k < 4; ++k)
    for (int l = 1; l < n_levels[k]; ++l) { lh[fh[k].level0 + l].img_off = bytes; bytes += rows[l] * (cols[l] + k); }
  return t.commit(std::move(fh), std::move(lh));
}

static void check_resident() {
  Keypoints kp(5, 4);
  osh_stereo_resident_frame f = kp.frame<osh_stereo_resident_frame>();
  check_validation<ResidentStereoLevels>(f, kp);

  PyramidTable t;
  const FastFrameHost *L = nullptr, *R = nullptr;
  CHECK(stereo_check_tokens("check", 2, nullptr, 1, 2, 3, &L, &R) == OSH_ERR_INVALID && said("check: frame 2: the token names no frame of this context's resident pyramid"));
  CHECK(stereo_check_tokens("check", 2, &t, 1, 2, 3, &L, &R) == OSH_ERR_INVALID && said("names no frame"));   // nothing committed yet
  const uint64_t T = commit_resident(t);
  CHECK(stereo_check_tokens("check", 0, &t, T, T + 1, 3, &L, &R) == OSH_OK && L == &t.frames[0] && R == &t.frames[1]);
  CHECK(stereo_check_tokens("check", 0, &t, T + 1, T, 3, &L, &R) == OSH_OK && L == &t.frames[1] && R == &t.frames[0]);
  CHECK(stereo_check_tokens("check", 0, &t, T, T, 3, &L, &R) == OSH_OK);
  CHECK(stereo_check_tokens("check", 0, &t, T, T + 4, 3, &L, &R) == OSH_ERR_INVALID && said("names no frame"));
  CHECK(stereo_check_tokens("check", 0, &t, 0, T, 3, &L, &R) == OSH_ERR_INVALID && said("names no frame"));
  CHECK(stereo_check_tokens("check", 1, &t, T + 2, T + 3, 3, &L, &R) == OSH_ERR_INVALID && said("frame 1: the left frame has 3 levels, the right frame 2, the call names 3"));
  CHECK(stereo_check_tokens("check", 1, &t, T, T + 1, 2, &L, &R) == OSH_ERR_INVALID && said("the left frame has 3 levels, the right frame 3, the call names 2"));
  CHECK(stereo_check_tokens("check", 1, &t, T + 3, T + 3, 2, &L, &R) == OSH_OK);

  // the plan of frames 2 (left) and 1 (right): sizes and offsets as the table has them, every level there
  StereoFrameDev d = stereo_frame_dev(5, 4, 0, 0, 3, 40.f, 1.f, kp.sf, kp.isf);
  stereo_plan_resident(t, t.frames[2], t.frames[1], d);
  CHECK(d.n_rows == 10 && d.rows_l[0] == 10 && d.cols_l[0] == 14 && d.cols_r[0] == 13 && d.rows_r[2] == 7 && d.cols_l[2] == 10 && d.cols_r[2] == 9);
  CHECK(d.off_l[0] == 10 * 12 + 10 * 13 && d.off_r[0] == 10 * 12);
  for (int l = 0; l < 3; ++l) CHECK(d.off_l[l] == t.levels[t.frames[2].level0 + l].img_off && d.off_r[l] == t.levels[t.frames[1].level0 + l].img_off);
  CHECK(d.off_l[3] == -1 && d.off_r[3] == -1 && d.rows_l[3] == 0);
  // after the pyramid is replaced the old tokens name nothing
  t.invalidate();
  CHECK(stereo_check_tokens("check", 0, &t, T, T + 1, 3, &L, &R) == OSH_ERR_INVALID && said("names no frame"));
  const uint64_t U = commit_resident(t);
  CHECK(stereo_check_tokens("check", 0, &t, T, T + 1, 3, &L, &R) == OSH_ERR_INVALID);
  CHECK(stereo_check_tokens("check", 0, &t, U, U + 1, 3, &L, &R) == OSH_OK);
  PyramidTable other;   // of another context: the counter is the process's
  const uint64_t V = commit_resident(other);
  CHECK(stereo_check_tokens("check", 0, &t, V, V + 1, 3, &L, &R) == OSH_ERR_INVALID && stereo_check_tokens("check", 0, &other, V, V + 1, 3, &L, &R) == OSH_OK);
}

// The slices of the row lists: every frame's holds what its right keypoints can enter, and a batch beyond the sizes is told apart
static void check_row_plan() {
  const float sf[3] = {1.f, 1.2f, 1.44f};
  StereoRowPlan p;
  StereoFrameDev a = stereo_frame_dev(5, 100, 0, 0, 3, 40.f, 1.f, sf, sf);
  a.n_rows = 480;
  StereoFrameDev b = stereo_frame_dev(5, 7, 5, 100, 1, 40.f, 1.f, sf, sf);
  b.n_rows = 4;        // fewer rows than a keypoint's span: clipped
  p.add(a); p.add(b);
  CHECK(p.fits() && p.frames.size() == 2 && p.rows == 484);
  CHECK(p.frames[0].row0 == 0 && p.frames[0].entry0 == 0 && p.frames[0].entry_end == 100 * 9);   // (int)(4 * 1.44 + 4) = 9 rows
  CHECK(p.frames[1].row0 == 480 && p.frames[1].entry0 == 900 && p.frames[1].entry_end == 900 + 7 * 4 && p.entries == 928);
  const float wild[2] = {1.f, NAN};
  StereoFrameDev c = stereo_frame_dev(1, 3, 0, 0, 2, 40.f, 1.f, wild, wild);
  c.n_rows = 50;
  p.add(c);
  CHECK(p.fits() && p.frames[2].entry_end - p.frames[2].entry0 == 150);   // a scale that is no number: every row
  StereoFrameDev huge = stereo_frame_dev(1, 1 << 22, 0, 0, 1, 40.f, 1.f, wild, wild);
  huge.n_rows = 32768; huge.sf[0] = 1.0e6f;
  p.add(huge);
  CHECK(!p.fits() && p.frames[3].entry_end == 0);
}

int main() {
  check_row_plan();
  check_brought();
  check_resident();
  std::printf(failures ? "FAILED: %d checks\n" : "stereo_frame_check ok\n", failures);
  return failures ? 1 : 0;
}
