// mappoint_check.cpp -- csrc/mappoint_refresh.h as plain C++ under AddressSanitizer and UBSan: a program of its own (make
// mappoint-check) that makes no HIP call and needs no device.  It runs the statements of MapPoint::ComputeDistinctiveDescriptors and
// MapPoint::UpdateNormalAndDepth on exactly-sized arrays at the extremes a valid call can carry: 0, 1, 2 and
// OSH_MAPPOINT_MAX_DESCRIPTORS entries and one more (the host build has no limit), all-zero against all-one descriptors (distance
// 256, the last bin of the counts), identical descriptors, no entry with use_desc, use_desc holes at both ends, a centre that is
// the point itself (norm 0) and coordinates near the float32 limits.  Every array has exactly the size the header may read, so a
// read past an end is an AddressSanitizer report.  It checks the results a definition gives without arithmetic.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../../include/orbslam3_hip.h"
#include "../mappoint_refresh.h"

static long checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::fprintf(stderr, "mappoint_check: line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

struct Case {
  std::vector<uint32_t> desc;
  std::vector<int32_t> centre;
  std::vector<uint8_t> use;
  std::vector<float> centres;
  osh::MpPoint p{};
  osh::MpOut run() {
    std::vector<uint16_t> table((size_t)p.n * p.n);   // exactly n * n
    osh::MpOut o;
    osh::mappoint_refresh_point(p, desc.data(), centre.data(), use.data(), centres.data(), table.data(), o);
    return o;
  }
};

// n entries whose descriptor words are word(i), centres on a circle of radius r around the origin, the point at `at`
template <class W>
static Case make(int n, W word, float r, float at) {
  Case c;
  c.p.n = n; c.p.pos[0] = at; c.p.pos[1] = 0.5f * at; c.p.pos[2] = -at; c.p.ref_centre = 0; c.p.level_scale = 1.728f; c.p.top_scale = 3.583f;
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 8; ++k) c.desc.push_back(word(i));
    c.centre.push_back(i % 7 == 3 ? 0 : i);   // a shared centre now and then
    c.use.push_back(1);
  }
  const int n_centres = n > 0 ? n : 1;
  for (int i = 0; i < n_centres; ++i) { c.centres.push_back(r * std::cos(0.1f * i)); c.centres.push_back(r * std::sin(0.1f * i)); c.centres.push_back(0.01f * i); }
  return c;
}

int main() {
  const int limit = OSH_MAPPOINT_MAX_DESCRIPTORS;
  for (int n : {0, 1, 2, 3, 4, 5, 63, 64, 65, limit, limit + 1}) {
    // identical descriptors: every row is all zeros, the first row wins
    Case same = make(n, [](int) { return 0xdeadbeefu; }, 2.f, 10.f);
    osh::MpOut o = same.run();
    if (n == 0) { CHECK(o.best_entry == -1 && o.best_median == -1 && o.normal[0] == 0.f && o.min_distance == 0.f && o.max_distance == 0.f); continue; }
    CHECK(o.best_entry == 0 && o.best_median == 0);
    CHECK(std::isfinite(o.normal[0]) && std::isfinite(o.normal[1]) && std::isfinite(o.normal[2]) && o.max_distance > o.min_distance && o.min_distance > 0.f);
    // all zeros against all ones, alternating: distance 256 lands in the last bin; with n even the median of every row is 0
    // (index (n - 1) / 2 of n / 2 zeros), with n odd the even rows have (n + 1) / 2 zeros and win with 0
    Case far = make(n, [](int i) { return i % 2 ? 0xffffffffu : 0u; }, 2.f, 10.f);
    o = far.run();
    CHECK(o.best_entry == 0 && o.best_median == 0);
    if (n >= 3) {   // one zero descriptor among ones: the first one-row wins with 0, and with n == 2 ... see above
      Case one = make(n, [](int i) { return i == 0 ? 0u : 0xffffffffu; }, 2.f, 10.f);
      o = one.run();
      CHECK(o.best_entry == 1 && o.best_median == 0);
      // the zero descriptor alone in use: M = 1
      for (int i = 1; i < n; ++i) one.use[i] = 0;
      o = one.run();
      CHECK(o.best_entry == 0 && o.best_median == 0);
      // holes at the first and the last entry: the winner is the first entry in use
      for (int i = 0; i < n; ++i) one.use[i] = i != 0 && i != n - 1;
      o = one.run();
      CHECK(o.best_entry == 1 && o.best_median == 0);
    }
    // no entry in use: the normal is still computed
    Case none = make(n, [](int i) { return (uint32_t)i * 2654435761u; }, 2.f, 10.f);
    for (int i = 0; i < n; ++i) none.use[i] = 0;
    o = none.run();
    CHECK(o.best_entry == -1 && o.best_median == -1 && std::isfinite(o.normal[2]) && o.max_distance > 0.f);
    // distances spread over all bins; the median of the winner lies in [0, 256]
    Case spread = make(n, [](int i) { return (uint32_t)i * 2654435761u; }, 2.f, 10.f);
    o = spread.run();
    CHECK(o.best_entry >= 0 && o.best_entry < n && o.best_median >= 0 && o.best_median <= 256);
    // coordinates near the float32 limits: squares overflow to infinity, nothing traps
    Case huge = make(n, [](int i) { return (uint32_t)i; }, 1.0e30f, 3.0e38f);
    o = huge.run();
    CHECK(o.best_entry >= 0);
    // the point on its reference centre: norm 0, a division by zero that IEEE defines
    Case zero = make(n, [](int i) { return (uint32_t)i; }, 0.f, 0.f);
    for (float& c : zero.centres) c = 0.f;
    o = zero.run();
    CHECK(o.max_distance == 0.f && std::isnan(o.normal[0]));
  }
  CHECK(osh::mp_median_index(1) == 0 && osh::mp_median_index(2) == 0 && osh::mp_median_index(3) == 1 && osh::mp_median_index(4) == 1 && osh::mp_median_index(5) == 2);
  std::printf("mappoint_check ok: %ld checks\n", checks);
  return 0;
}
