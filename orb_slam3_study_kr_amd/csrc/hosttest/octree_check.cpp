// octree_check.cpp -- csrc/orb_octree.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make octree-check) that
// makes no HIP call and needs no device.  It runs osh::octree_distribute_host and osh::oct_validate_list on candidate arrays
// allocated at exactly their size: empty and one-candidate lists, N of 0, 1, negative and beyond the candidates, portrait areas
// (nIni == 0), wide areas with several roots, a one-row area with as many roots as columns, candidates on one pixel, below the area
// and on the last representable x below the width, dense clusters that go through round B more than once, and the largest sides.  It
// checks that every list ends (no list reaches kOctMaxRounds), that the kept indices are distinct and in range, that their count
// respects max(N + 3, 4 nIni) and the candidate count, the known answers of a hand-computed list and of the lone-quadrant list,
// and what the validator refuses.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../orb_octree.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int run_list(const char* what, const std::vector<float>& xy, const std::vector<float>& response, int W, int H, int N, std::vector<int>& kept) {
  const int n = (int)response.size();
  const char* why = "";
  if (osh::oct_validate_list(n, n ? xy.data() : nullptr, n ? response.data() : nullptr, W, H, N, &why) == osh::kOctInvalid) { std::printf("%s: refused: %s\n", what, why); return 1; }
  const int rc = osh::octree_distribute_host(n, xy.data(), response.data(), W, H, N, kept);
  if (rc != osh::kOctOk) { std::printf("%s: status %d\n", what, rc); return 1; }
  const int n_ini = osh::oct_n_ini(W, H);
  const long bound = std::max<long>((long)N + 3, 4L * n_ini);
  if ((long)kept.size() > bound || (int)kept.size() > n || (n > 0 && kept.empty())) { std::printf("%s: %zu kept of %d, N = %d, nIni = %d\n", what, kept.size(), n, N, n_ini); return 1; }
  std::vector<char> seen(n, 0);
  for (int k : kept) {
    if (k < 0 || k >= n || seen[k]) { std::printf("%s: index %d out of range or kept twice\n", what, k); return 1; }
    seen[k] = 1;
  }
  return 0;
}

static int random_list(int n, int W, int H, int N, int kind) {
  std::vector<float> xy((size_t)n * 2), response(n);
  for (int k = 0; k < n; ++k) {
    float x, y;
    switch (kind) {
      case 0: x = (float)(rng() % (uint32_t)W); y = (float)(rng() % (uint32_t)H); break;                                  // pixels
      case 1: x = (float)W * (float)(rng() % 4096u) / 4096.f; y = (float)H * (float)(rng() % 4096u) / 2048.f; break;      // fractional, some below the area
      case 2: x = (float)((rng() % 5u) * (uint32_t)W / 5u + rng() % 3u); y = (float)((rng() % 3u) * (uint32_t)H / 3u + rng() % 2u); break;   // clusters of 3 x 2 pixels
      default: x = std::nextafter((float)W, 0.f); y = (float)(rng() % 2u); break;                                          // the last x below the width
    }
    if (!(x < (float)W)) x = std::nextafter((float)W, 0.f);
    xy[2 * k] = x; xy[2 * k + 1] = y;
    response[k] = (float)(rng() % 9u);
  }
  std::vector<int> kept;
  char what[96];
  std::snprintf(what, sizeof what, "n %d area %dx%d N %d kind %d", n, W, H, N, kind);
  return run_list(what, xy, response, W, H, N, kept);
}

int main() {
  int bad = 0;
  long lists = 0;
  const int areas[][2] = {{128, 88}, {300, 100}, {150, 100}, {40, 100}, {1, 1}, {1, 300}, {300, 1}, {720, 448}, {32768, 1}, {1, 32768}, {32768, 32768}, {7, 3}};
  const int counts[] = {0, 1, 2, 3, 17, 64, 65, 500};
  const int wanted[] = {-3, 0, 1, 2, 20, 217, 2048, 100000};
  for (const auto& a : areas)
    for (int n : counts)
      for (int N : wanted)
        for (int kind = 0; kind < 4; ++kind) { bad += random_list(n, a[0], a[1], N, kind); ++lists; }
  bad += random_list(3000, 720, 448, 217, 0); bad += random_list(3000, 720, 448, 217, 2); bad += random_list(70000, 752, 480, 3000, 0);
  lists += 3;

  // known answers.  One root over 128 x 88, four candidates in one quadrant: the list does not grow, the strongest is kept, the first of two equals
  std::vector<int> kept;
  bad += run_list("lone quadrant", {3, 2, 10, 20, 40, 30, 63, 43}, {5, 9, 9, 1}, 128, 88, 10, kept);
  if (kept != std::vector<int>{1}) { std::printf("lone quadrant: kept %zu\n", kept.size()); ++bad; }
  // 100 x 100, one root, mid 50: one candidate per quadrant; pushed to the front in the order n1 .. n4, the list reads n4, n3, n2, n1
  bad += run_list("four quadrants", {10, 10, 60, 10, 10, 60, 60, 60}, {1, 2, 3, 4}, 100, 100, 4, kept);
  if (kept != std::vector<int>{3, 2, 1, 0}) { std::printf("four quadrants: wrong order\n"); ++bad; }
  // two candidates on one pixel and N = 5: every round divides their node and the list stays at one node
  bad += run_list("one pixel", {70, 50, 70, 50}, {4, 6}, 128, 88, 5, kept);
  if (kept != std::vector<int>{1}) { std::printf("one pixel: kept %zu\n", kept.size()); ++bad; }
  // 300 x 100: three roots [0, 100) [100, 200) [200, 300); x = 100 belongs to the second, N = 0 stops after the first round
  bad += run_list("three roots", {99, 5, 100, 5, 250, 5}, {1, 1, 1}, 300, 100, 0, kept);
  if (kept != std::vector<int>{0, 1, 2}) { std::printf("three roots: wrong order\n"); ++bad; }
  lists += 4;

  // the validator
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const char* why = "";
  const float one_xy[2] = {1, 1}, one_r[1] = {1};
  struct { float x, y, r; int W, H, N, n; int expect; } refusals[] = {
      {1, 1, 1, 10, 10, 5, 1, osh::kOctOk},         {nan, 1, 1, 10, 10, 5, 1, osh::kOctInvalid},  {1, inf, 1, 10, 10, 5, 1, osh::kOctInvalid},
      {1, 1, nan, 10, 10, 5, 1, osh::kOctInvalid},  {10, 1, 1, 10, 10, 5, 1, osh::kOctInvalid},   {-1, 1, 1, 10, 10, 5, 1, osh::kOctInvalid},
      {1, -1, 1, 10, 10, 5, 1, osh::kOctInvalid},   {1, 50, 1, 10, 10, 5, 1, osh::kOctOk},        {1, 1, 1, 0, 10, 5, 1, osh::kOctInvalid},
      {1, 1, 1, 10, 32769, 5, 1, osh::kOctInvalid}, {1, 1, 1, 10, 10, 2049, 1, osh::kOctUnsupported}, {1, 1, 1, 10, 10, 2048, 1, osh::kOctOk},
      {1, 1, 1, 650, 10, 5, 1, osh::kOctUnsupported}, {1, 1, 1, 10, 10, 5, -1, osh::kOctInvalid}};
  for (const auto& c : refusals) {
    const float cxy[2] = {c.x, c.y}, cr[1] = {c.r};
    if (osh::oct_validate_list(c.n, cxy, cr, c.W, c.H, c.N, &why) != c.expect) { std::printf("validator: (%g, %g, %g) in %dx%d N %d n %d\n", c.x, c.y, c.r, c.W, c.H, c.N, c.n); ++bad; }
  }
  if (osh::oct_validate_list(1, nullptr, one_r, 10, 10, 5, &why) != osh::kOctInvalid || osh::oct_validate_list(1, one_xy, nullptr, 10, 10, 5, &why) != osh::kOctInvalid ||
      osh::oct_validate_list(0, nullptr, nullptr, 10, 10, 5, &why) != osh::kOctOk || osh::oct_validate_list(65537, nullptr, nullptr, 10, 10, 5, &why) != osh::kOctInvalid) { std::printf("validator: NULL arrays\n"); ++bad; }
  std::printf("octree_check: %ld lists, %d failures\n", lists, bad);
  return bad ? 1 : 0;
}
