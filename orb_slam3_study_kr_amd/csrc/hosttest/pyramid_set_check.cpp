// pyramid_set_check.cpp -- PyramidTable, PyramidLevels and validate_keypoints of csrc/orb_pyramid_set.h on plain host memory, for a run
// under a sanitizer: calls that mix brought pyramids and a token in every order, listed, staged into a malloc'ed stand-in of the
// upload of exactly img_bytes and indexed into one of exactly the keypoint count; the token lookup through commit and invalidate;
// the keypoint check on the limit of its reach.  A program of its own (`make pyramid-set-check`), in no library; it makes no HIP
// call and needs no device.
#include <cstdio>
#include <string>
#include <vector>

#include "../orb_pyramid_set.h"

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
#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// A level of its own allocation, exactly as long as its last row needs
struct Image {
  int rows, cols, stride;
  unsigned char* data;
  Image(int rows_, int cols_, int stride_, int seed) : rows(rows_), cols(cols_), stride(stride_) {
    const size_t bytes = (size_t)(rows - 1) * stride + cols;
    data = static_cast<unsigned char*>(std::malloc(bytes));
    for (size_t i = 0; i < bytes; ++i) data[i] = (unsigned char)(seed + 3 * i);
  }
  Image(const Image&) = delete;
  ~Image() { std::free(data); }
  osh_stereo_image view() const { return {data, rows, cols, stride}; }
};

// The resident table as a build lays it out: the level 0 of both frames first, then the other levels frame after frame
static const int kResRows[2][3] = {{6, 5, 4}, {4, 3, 0}}, kResCols[2][3] = {{8, 7, 6}, {4, 3, 0}}, kResLevels[2] = {3, 2};
static const long long kResOff[2][3] = {{0, 64, 99}, {48, 123, 0}};
static const size_t kResBytes = 132;

static uint64_t commit_resident(PyramidTable& t) {
  std::vector<FastFrameHost> fh;
  std::vector<FastLevelHost> lh;
  for (int k = 0; k < 2; ++k) {
    fh.push_back({(int)lh.size(), kResLevels[k], 0, 0});
    for (int l = 0; l < kResLevels[k]; ++l) lh.push_back({kResOff[k][l], kResRows[k][l], kResCols[k][l], 0, 0});
  }
  return t.commit(std::move(fh), std::move(lh));
}

// One call: `order` names its frames, 'A' (brings 5x7 stride 9 and 3x4 stride 4), 'B' (brings 1x1) and 'T' (frame 1 of the table)
template <class Frame>
static void check_call(const char* order) {
  const Image a0(5, 7, 9, 1), a1(3, 4, 4, 2), b0(1, 1, 1, 3);
  const osh_stereo_image pyr_a[2] = {a0.view(), a1.view()}, pyr_b[1] = {b0.view()};
  const int32_t level_a[3] = {1, 0, 1}, level_b[1] = {0}, level_t[2] = {1, 0};
  PyramidTable table;
  const uint64_t token0 = commit_resident(table);
  const int n_frames = (int)std::string(order).size();
  bool any_token = false;
  std::vector<Frame> frames(n_frames);
  for (int k = 0; k < n_frames; ++k) {
    Frame& f = frames[k];
    f = Frame{};
    if (order[k] == 'A') { f.n_levels = 2; f.pyramid = pyr_a; f.n = 3; f.level = level_a; }
    if (order[k] == 'B') { f.n_levels = 1; f.pyramid = pyr_b; f.n = 1; f.level = level_b; }
    if (order[k] == 'T') { f.pyramid_token = token0 + 1; f.n = 2; f.level = level_t; any_token = true; }
  }
  const PyramidTable* rp = any_token ? &table : nullptr;   // a call without a token frame never asks for the table

  PyramidLevels<Frame> pl{"check", n_frames, frames.data()};
  std::string seen;
  const auto sizes = [&](int k, int n, const PyramidLevel* sz) {   // the validator of the entry: here it checks what it is handed
    seen += order[k];
    if (order[k] == 'A') CHECK(n == 2 && sz[0].rows == 5 && sz[0].cols == 7 && sz[1].rows == 3 && sz[1].cols == 4 && !sz[0].resident && !sz[1].resident);
    if (order[k] == 'B') CHECK(n == 1 && sz[0].rows == 1 && sz[0].cols == 1 && !sz[0].resident);
    if (order[k] == 'T') CHECK(n == 2 && sz[0].rows == 4 && sz[0].cols == 4 && sz[1].rows == 3 && sz[1].cols == 3 && sz[0].resident && sz[1].resident);
    return (int)OSH_OK;
  };
  CHECK(pl.check_brought(sizes) == OSH_OK && pl.any_token == any_token);
  CHECK(pl.check_tokens(rp, sizes) == OSH_OK);
  std::string brought_first;   // the two-pass order: every brought frame before any token frame
  for (int pass = 0; pass < 2; ++pass)
    for (int k = 0; k < n_frames; ++k) if ((order[k] == 'T') == (pass == 1)) brought_first += order[k];
  CHECK(seen == brought_first);
  CHECK(pl.list(rp) == OSH_OK);

  // the list against a walk of its own
  size_t at = 0, img_bytes = 0, n_keypoints = 0;
  for (int k = 0; k < n_frames; ++k) {
    CHECK(pl.level0[k] == (int)at);
    if (order[k] == 'T') {
      CHECK(pl.n_levels[k] == 2);
      for (int l = 0; l < 2; ++l) CHECK(pl.lv[at + l].resident && pl.lv[at + l].off == (size_t)kResOff[1][l] && pl.lv[at + l].rows == kResRows[1][l] && pl.lv[at + l].cols == kResCols[1][l]);
    } else {
      CHECK(pl.n_levels[k] == frames[k].n_levels);
      for (int l = 0; l < frames[k].n_levels; ++l) {
        const osh_stereo_image& im = frames[k].pyramid[l];
        CHECK(!pl.lv[at + l].resident && pl.lv[at + l].off == img_bytes && pl.lv[at + l].rows == im.rows && pl.lv[at + l].cols == im.cols);
        img_bytes += (size_t)im.rows * im.cols;
      }
    }
    at += (size_t)pl.n_levels[k];
    n_keypoints += (size_t)frames[k].n;
  }
  CHECK(pl.lv.size() == at && pl.img_bytes == img_bytes);

  // staging: the source rows with the stride removed, into exactly img_bytes
  unsigned char* staged = static_cast<unsigned char*>(std::malloc(img_bytes));
  pl.stage(staged);
  for (int k = 0; k < n_frames; ++k)
    for (int l = 0; frames[k].pyramid && l < frames[k].n_levels; ++l) {
      const osh_stereo_image& im = frames[k].pyramid[l];
      const unsigned char* dst = staged + pl.lv[pl.level0[k] + l].off;
      for (int r = 0; r < im.rows; ++r) CHECK(std::memcmp(dst + (size_t)r * im.cols, im.data + (size_t)r * im.stride, (size_t)im.cols) == 0);
    }
  // device pointers: the base of the level's side plus its offset (stand-ins; never dereferenced)
  unsigned char* resident = any_token ? static_cast<unsigned char*>(std::malloc(kResBytes)) : nullptr;
  for (size_t l = 0; l < pl.lv.size(); ++l) {
    CHECK(pl.data(l, resident, staged) == (pl.lv[l].resident ? resident : staged) + pl.lv[l].off);
    CHECK(pl.lv[l].off + (size_t)pl.lv[l].rows * pl.lv[l].cols <= (pl.lv[l].resident ? kResBytes : img_bytes));
  }
  // every keypoint's entry of the list, into exactly n_keypoints ints
  int* index = static_cast<int*>(std::malloc(n_keypoints * sizeof(int)));
  pl.index(index);
  size_t i = 0;
  for (int k = 0; k < n_frames; ++k)
    for (int j = 0; j < frames[k].n; ++j, ++i) CHECK(index[i] == pl.level0[k] + frames[k].level[j]);
  std::free(index); std::free(resident); std::free(staged);
  std::printf("pyramid_set_check: frames %s: %zu levels, %zu bytes brought, %zu keypoints\n", order, at, img_bytes, n_keypoints);
}

static void check_refusals_of_the_list() {
  PyramidTable table;
  const uint64_t token0 = commit_resident(table);
  const auto ok = [](int, int, const PyramidLevel*) { return (int)OSH_OK; };
  osh_ic_angle_frame stale{};
  stale.pyramid_token = token0 + 2;
  PyramidLevels<osh_ic_angle_frame> pl{"check", 1, &stale};
  CHECK(pl.check_brought(ok) == OSH_OK && pl.any_token);
  CHECK(pl.check_tokens(&table, ok) == OSH_ERR_INVALID && std::strstr(last_error, "check: frame 0: the token names no frame of this context's resident pyramid"));
  // three levels of 2^30 bytes: described only, list() reads no pixel
  unsigned char pixel = 0;
  const osh_stereo_image big[3] = {{&pixel, 32768, 32768, 32768}, {&pixel, 32768, 32768, 32768}, {&pixel, 32768, 32768, 32768}};
  osh_ic_angle_frame huge{};
  huge.n_levels = 3; huge.pyramid = big;
  PyramidLevels<osh_ic_angle_frame> pb{"check", 1, &huge};
  CHECK(pb.check_brought(ok) == OSH_OK && !pb.any_token);
  CHECK(pb.list(nullptr) == OSH_ERR_UNSUPPORTED && std::strstr(last_error, "batch too large"));
  huge.n_levels = 2;   // 2^31 exactly is within the limit
  PyramidLevels<osh_ic_angle_frame> pc{"check", 1, &huge};
  CHECK(pc.list(nullptr) == OSH_OK && pc.img_bytes == (size_t)1 << 31);
}

static void check_tokens() {
  PyramidTable t;
  CHECK(!t.frame(0) && !t.frame(1));
  const uint64_t T = commit_resident(t);
  CHECK(T != 0 && t.frame(T) == &t.frames[0] && t.frame(T + 1) == &t.frames[1]);
  CHECK(!t.frame(0) && !t.frame(T - 1) && !t.frame(T + 2) && !t.frame((uint64_t)1 << 63));
  t.invalidate();
  CHECK(!t.frame(T) && !t.frame(T + 1) && !t.frame(0));
  const uint64_t U = commit_resident(t);
  CHECK(U >= T + 2 && !t.frame(T) && !t.frame(T + 1) && t.frame(U) == &t.frames[0] && t.frame(U + 1) == &t.frames[1]);
  PyramidTable other;   // of another context: the counter is the process's
  const uint64_t V = commit_resident(other);
  CHECK(V >= U + 2 && !t.frame(V) && !other.frame(U));
}

static void check_keypoints() {
  const PyramidLevel one{false, 0, 31, 31};
  const auto rc = [&](float x, float y, int32_t level) {
    const float xy[2] = {x, y};
    return validate_keypoints("check", 4, 1, xy, &level, 1, &one, 15, "disc");
  };
  CHECK(rc(15.f, 15.f, 0) == OSH_OK);
  CHECK(rc(15.4f, 14.6f, 0) == OSH_OK);   // rounds to the centre
  CHECK(rc(14.4f, 15.f, 0) == OSH_ERR_INVALID && std::strstr(last_error, "check: frame 4: keypoint 0: the 31-pixel disc leaves level 0"));
  CHECK(rc(15.f, 15.6f, 0) == OSH_ERR_INVALID && std::strstr(last_error, "the 31-pixel disc leaves level 0"));
  CHECK(rc(NAN, 15.f, 0) == OSH_ERR_INVALID && std::strstr(last_error, "keypoint 0 is not finite"));
  CHECK(rc(15.f, INFINITY, 0) == OSH_ERR_INVALID && std::strstr(last_error, "keypoint 0 is not finite"));
  CHECK(rc(15.f, 15.f, -1) == OSH_ERR_INVALID && std::strstr(last_error, "level -1 outside [0, 1)"));
  CHECK(rc(15.f, 15.f, 1) == OSH_ERR_INVALID && std::strstr(last_error, "level 1 outside [0, 1)"));
  CHECK(rc(3e9f, 15.f, 0) == OSH_ERR_INVALID && std::strstr(last_error, "leaves level 0"));   // never converted to int
  CHECK(rc(15.f, -3e9f, 0) == OSH_ERR_INVALID && std::strstr(last_error, "leaves level 0"));
}

int main() {
  check_call<osh_ic_angle_frame>("ATB");
  check_call<osh_ic_angle_frame>("TAB");
  check_call<osh_describe_frame>("ABT");
  check_call<osh_describe_frame>("T");     // nothing brought: img_bytes == 0
  check_call<osh_ic_angle_frame>("AB");    // no token: no table and no resident pointer
  check_refusals_of_the_list();
  check_tokens();
  check_keypoints();
  std::printf(failures ? "FAILED: %d checks\n" : "pyramid_set_check ok\n", failures);
  return failures ? 1 : 0;
}
