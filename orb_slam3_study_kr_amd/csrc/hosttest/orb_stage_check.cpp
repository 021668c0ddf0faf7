// orb_stage_check.cpp -- KeypointBatch and scatter of csrc/orb_stage.h on plain host memory, for a run under a sanitizer: the batches
// of tests/test_gpu_stereo_shared_ctx.py for both frame types, staged into a malloc'ed stand-in of the pinned buffer of exactly the
// Layout's size, compared with the inputs, and results scattered back from a stand-in of the downloaded outputs.  A program of its
// own (`make stage-check`), in no library; it makes no HIP call and needs no device.
#include <cstdio>
#include <numeric>
#include <vector>

#include "../orb_stage.h"

namespace osh {
void set_error(const char*, ...) {}
}  // namespace osh
using namespace osh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Side {
  std::vector<float> xy;
  std::vector<int32_t> octave;
  std::vector<uint8_t> desc;
  Side(int n, int seed) : xy(2 * (size_t)n), octave(n), desc(32 * (size_t)n) {
    std::iota(xy.begin(), xy.end(), 1000.f * seed);
    std::iota(octave.begin(), octave.end(), 100 * seed);
    for (size_t i = 0; i < desc.size(); ++i) desc[i] = (uint8_t)(i * 7 + seed);
  }
};

template <class Frame>
static void check(const char* what, const std::vector<std::pair<int, int>>& counts) {
  const int n_frames = (int)counts.size();
  std::vector<Side> left, right;
  std::vector<Frame> frames(n_frames);
  for (int k = 0; k < n_frames; ++k) { left.emplace_back(counts[k].first, 2 * k + 1); right.emplace_back(counts[k].second, 2 * k + 2); }
  for (int k = 0; k < n_frames; ++k) {
    Frame& f = frames[k];
    f.n_left = counts[k].first; f.n_right = counts[k].second;
    // an empty side hands over NULL, as a caller may
    f.left_xy = f.n_left ? left[k].xy.data() : nullptr; f.left_octave = f.n_left ? left[k].octave.data() : nullptr; f.left_desc = f.n_left ? left[k].desc.data() : nullptr;
    f.right_xy = right[k].xy.data(); f.right_octave = right[k].octave.data(); f.right_desc = right[k].desc.data();
  }
  KeypointBatch kb;
  CHECK(kb.size(what, n_frames, frames.data()) == OSH_OK);
  Layout in, out;
  in.take<double>(n_frames);   // the entry's frame descriptors come first
  kb.take(in);
  const auto o_one = out.take<int>(kb.NL);
  const auto o_three = out.take<float>(kb.NL * 3);
  const auto o_right = out.take<int>(kb.NR);
  char* h_in = static_cast<char*>(std::malloc(in.bytes));
  char* h_out = static_cast<char*>(std::malloc(out.bytes));
  kb.stage(h_in, frames.data());
  size_t nl = 0, nr = 0;
  int max_left = 0, max_right = 0;
  for (int k = 0; k < n_frames; ++k) {
    CHECK(kb.base[k].left == (int)nl && kb.base[k].right == (int)nr);
    const size_t L = (size_t)counts[k].first, R = (size_t)counts[k].second;
    CHECK(L == 0 || std::memcmp(kb.lxy.in(h_in) + nl, left[k].xy.data(), L * 8) == 0);
    CHECK(L == 0 || std::memcmp(kb.loct.in(h_in) + nl, left[k].octave.data(), L * 4) == 0);
    CHECK(L == 0 || std::memcmp(kb.ldesc.in(h_in) + nl * 2, left[k].desc.data(), L * 32) == 0);
    CHECK(R == 0 || std::memcmp(kb.rxy.in(h_in) + nr, right[k].xy.data(), R * 8) == 0);
    CHECK(R == 0 || std::memcmp(kb.roct.in(h_in) + nr, right[k].octave.data(), R * 4) == 0);
    CHECK(R == 0 || std::memcmp(kb.rdesc.in(h_in) + nr * 2, right[k].desc.data(), R * 32) == 0);
    nl += L; nr += R;
    max_left = std::max(max_left, counts[k].first); max_right = std::max(max_right, counts[k].second);
  }
  CHECK(kb.NL == nl && kb.NR == nr && kb.max_left == max_left && kb.max_right == max_right);
  // results: item i of the batch holds i (one per item), 3 i + c (three per item), -i (right side)
  for (size_t i = 0; i < nl; ++i) { o_one.in(h_out)[i] = (int)i; for (int c = 0; c < 3; ++c) o_three.in(h_out)[3 * i + c] = (float)(3 * i + c); }
  for (size_t i = 0; i < nr; ++i) o_right.in(h_out)[i] = -(int)i;
  const char* ho = h_out;
  for (int k = 0; k < n_frames; ++k) {
    const size_t L = (size_t)counts[k].first, R = (size_t)counts[k].second, bl = (size_t)kb.base[k].left, br = (size_t)kb.base[k].right;
    std::vector<int> one(L, -7), rgt(R, 7);
    std::vector<float> three(3 * L, -7.f);
    scatter(one.data(), o_one, ho, bl, L);
    scatter(three.data(), o_three, ho, bl, L, 3);
    scatter(rgt.data(), o_right, ho, br, R);
    scatter(static_cast<int*>(nullptr), o_one, ho, bl, L);   // an output the caller did not ask for
    for (size_t i = 0; i < L; ++i) { CHECK(one[i] == (int)(bl + i)); for (int c = 0; c < 3; ++c) CHECK(three[3 * i + c] == (float)(3 * (bl + i) + c)); }
    for (size_t i = 0; i < R; ++i) CHECK(rgt[i] == -(int)(br + i));
  }
  std::free(h_in); std::free(h_out);
  std::printf("%s: %d frames, %zu + %zu keypoints\n", what, n_frames, nl, nr);
}

int main() {
  check<osh_stereo_frame>("rectified", {{65, 257}, {0, 40}});
  check<osh_stereo_frame>("rectified, one frame", {{700, 3}});
  check<osh_fisheye_stereo_frame>("fisheye", {{64, 256}, {1, 2}});
  CHECK(right_set_slices(2, 2, 257, 256) == 2 && right_set_slices(11, 1, 3, 256) == 1 && right_set_slices(0, 2, 0, 256) == 1 &&
        right_set_slices(16, 1, 1000, 256) == 4 && right_set_slices(1, 1, 100000, 256) == 16);
  osh_stereo_frame big{};
  big.n_left = INT_MAX / 16 + 1;
  KeypointBatch kb;
  CHECK(kb.size("too large", 1, &big) == OSH_ERR_UNSUPPORTED);
  std::printf(failures ? "FAILED: %d checks\n" : "orb_stage_check ok\n", failures);
  return failures ? 1 : 0;
}
