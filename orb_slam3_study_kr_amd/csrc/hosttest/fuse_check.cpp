// fuse_check.cpp -- csrc/orb_fuse.h and csrc/orb_grid_bin.h as plain C++ under AddressSanitizer and UBSan: a program of its own
// (make fuse-check) that makes no HIP call and needs no device.  It runs the per-pair statements of ORBmatcher::Fuse on exactly-sized
// arrays at the extremes a valid call can carry: 0 and 1 points, a target without keypoints, OSH_FUSE_MAX_KEYS keypoints,
// OSH_FUSE_MAX_CELL_ENTRIES of them in one cell, a grid of OSH_FUSE_MAX_CELLS cells, OSH_FUSE_MAX_TARGETS targets, OSH_FUSE_MAX_LEVELS
// levels, a window clipped at each of the four grid edges and one that covers the whole grid, NaN and infinite positions and
// distance ranges, th = 0, th = 1e6 and th near the float32 limit.  Every array has exactly the size the headers may read, so a read past an
// end is an AddressSanitizer report, and a float that no int holds must not reach a conversion.  It checks the results a definition
// gives without arithmetic.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../orb_fuse.h"
#include "../orb_grid_bin.h"

static long checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::fprintf(stderr, "fuse_check: line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

struct Target {
  osh::FuseTarget T{};
  std::vector<float> xy, uright;
  std::vector<int> octave, coff, cidx;
  std::vector<uint32_t> desc;
  int most = 0;
  // identity pose at the origin, fx = fy = 256, cx = 320, cy = 240, the image 640 x 480, cells of 640 / cols x 480 / rows pixels
  Target(int cols, int rows, int n_levels, float th) {
    T.R[0] = T.R[4] = T.R[8] = 1.f;
    T.fx = T.fy = 256.f; T.cx = 320.f; T.cy = 240.f; T.bf = 40.f;
    T.min_x = 0.f; T.max_x = 640.f; T.min_y = 0.f; T.max_y = 480.f;
    T.winv = (float)cols / 640.f; T.hinv = (float)rows / 480.f; T.cols = cols; T.rows = rows;
    T.camera = OSH_FUSE_PINHOLE; T.n_levels = n_levels; T.log_sf = std::log(1.2f); T.th = th;
    for (int k = 0; k < n_levels; ++k) { T.scale[k] = k ? T.scale[k - 1] * 1.2f : 1.f; T.inv_sigma2[k] = 1.f / (T.scale[k] * T.scale[k]); }
  }
  void add(float x, float y, int oct, uint32_t word, float ur = -1.f) {
    xy.push_back(x); xy.push_back(y); octave.push_back(oct); uright.push_back(ur);
    for (int k = 0; k < 8; ++k) desc.push_back(word);
  }
  osh::FuseKeys bin(bool stereo) {
    const int n = (int)octave.size();
    T.n_keys = n; T.has_uright = stereo;
    coff.assign((size_t)T.cols * T.rows + 1, 0);
    cidx.assign((size_t)n, 0);                                        // exactly n: empty for a target without keypoints
    std::vector<int> cell_of, fill;
    most = osh::bin_keypoints(xy.data(), n, T.grid_min_x, T.grid_min_y, T.winv, T.hinv, T.cols, T.rows, OSH_FUSE_MAX_CELL_ENTRIES, coff.data(), cidx.data(), cell_of, fill);
    return osh::FuseKeys{xy.data(), octave.data(), stereo ? uright.data() : nullptr, desc.data(), coff.data(), cidx.data()};
  }
};

struct Out { osh::FuseGeom g; osh::FuseFound f; };

static Out run(const Target& t, const osh::FuseKeys& keys, const std::vector<float>& pos, const std::vector<float>& normal, float min_d, float max_d, int mode,
               bool skip = false) {
  const std::vector<uint32_t> q(8, 0u);                               // exactly one descriptor
  Out o{};
  o.f = {0, 0, -1, 256};
  osh::fuse_project(t.T, pos.data(), normal.data(), min_d, max_d, skip, o.g);
  if (o.g.stage == OSH_FUSE_SEARCHED) {
    o.f = osh::fuse_scan(t.T, keys, o.g, q.data(), mode);
    if (o.f.n_in == 0) o.g.stage = OSH_FUSE_EMPTY;
  }
  return o;
}

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const std::vector<float> axis = {0.f, 0.f, 1.f};
  for (int mode : {OSH_FUSE_CHI2, OSH_FUSE_SIM3}) {
    {   // a target without keypoints, one point: nothing is read from the empty arrays
      Target t(64, 48, 8, 3.f);
      const osh::FuseKeys k = t.bin(false);
      CHECK(t.most == 0);
      const Out o = run(t, k, {0.f, 0.f, 2.f}, axis, 0.1f, 2.f, mode);
      CHECK(o.g.stage == OSH_FUSE_EMPTY && o.g.level == 0 && o.g.radius == 3.f && o.f.best_idx == -1 && o.f.best_dist == 256);
      CHECK(run(t, k, {0.f, 0.f, 2.f}, axis, 0.1f, 2.f, mode, true).g.stage == OSH_FUSE_SKIPPED);
    }
    {   // windows clipped at the four edges, a keypoint in each; the corner pixels of the image
      Target t(64, 48, 8, 3.f);
      t.add(1.f, 176.f, 0, 1u); t.add(634.9f, 176.f, 0, 3u); t.add(256.f, 1.f, 0, 7u); t.add(256.f, 474.9f, 0, 15u);
      const osh::FuseKeys k = t.bin(false);
      const float px[4][3] = {{-2.49f, -0.5f, 2.f}, {2.4765625f, -0.5f, 2.f}, {-0.5f, -1.87f, 2.f}, {-0.5f, 1.8515625f, 2.f}};
      for (int e = 0; e < 4; ++e) {
        const std::vector<float> p(px[e], px[e] + 3);
        const float d = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        const Out o = run(t, k, p, axis, 0.1f, d, mode);
        CHECK(o.g.stage == OSH_FUSE_SEARCHED && o.f.best_idx == e && o.f.best_dist == 8 * (e + 1) && o.f.n_candidates == 1);
      }
      for (float x : {-2.5f, 2.4999f}) for (float y : {-1.875f, 1.8749f}) {
        const Out o = run(t, k, {x, y, 2.f}, axis, 0.1f, 4.f, mode);
        CHECK(o.g.stage == OSH_FUSE_EMPTY || o.g.stage == OSH_FUSE_SEARCHED);
      }
      // positions and ranges that are not finite: a gate fails or the level is clamped, nothing traps
      CHECK(run(t, k, {nan, 0.f, 2.f}, axis, 0.1f, 2.f, mode).g.stage == OSH_FUSE_OUTSIDE);
      CHECK(run(t, k, {0.f, 0.f, nan}, axis, 0.1f, 2.f, mode).g.stage == OSH_FUSE_OUTSIDE);
      CHECK(run(t, k, {inf, 0.f, 2.f}, axis, 0.1f, 2.f, mode).g.stage == OSH_FUSE_OUTSIDE);
      CHECK(run(t, k, {0.f, 0.f, inf}, axis, 0.1f, 2.f, mode).g.stage == OSH_FUSE_OUTSIDE);   // 0 * inf in the rotation
      CHECK(run(t, k, {0.f, 0.f, 0.f}, axis, 0.1f, 2.f, mode).g.stage == OSH_FUSE_OUTSIDE);
      CHECK(run(t, k, {0.f, 0.f, 2.f}, axis, nan, nan, mode).g.level == 0);
      CHECK(run(t, k, {0.f, 0.f, 2.f}, axis, 0.f, inf, mode).g.level == 0);
      CHECK(run(t, k, {0.f, 0.f, 2.f}, {nan, nan, nan}, 0.1f, 2.f, mode).g.stage >= OSH_FUSE_EMPTY);
      CHECK(run(t, k, {0.f, 0.f, 1e-30f}, axis, 0.f, 1e38f, mode).g.level == 0);   // dist underflows to 0: the ratio is infinite
    }
    for (float th : {0.f, -1.f, 1.0e6f, 3.0e38f}) {   // no radius; a huge one: the whole grid; one no int holds: INT_MIN in the reference's build, an early return
      Target t(64, 48, OSH_FUSE_MAX_LEVELS, th);
      for (int i = 0; i < 100; ++i) t.add(6.4f * i + 1.f, 4.7f * i + 1.f, i % OSH_FUSE_MAX_LEVELS, (uint32_t)i);
      const osh::FuseKeys k = t.bin(true);
      const Out o = run(t, k, {0.f, 0.f, 2.f}, axis, 0.1f, 2.f * t.T.scale[OSH_FUSE_MAX_LEVELS - 1], mode);
      CHECK(o.g.level == OSH_FUSE_MAX_LEVELS - 1);
      if (th == 1.0e6f) CHECK(o.g.stage == OSH_FUSE_SEARCHED && o.f.n_in == 100); else CHECK(o.g.stage == OSH_FUSE_EMPTY);
    }
    {   // OSH_FUSE_MAX_CELLS cells, OSH_FUSE_MAX_KEYS keypoints, OSH_FUSE_MAX_CELL_ENTRIES of them in one cell and one more in another
      Target t(128, 128, 8, 3.f);
      CHECK(t.T.cols * t.T.rows == OSH_FUSE_MAX_CELLS);
      for (int i = 0; i < OSH_FUSE_MAX_CELL_ENTRIES; ++i) t.add(320.f + 0.001f * i, 240.f, 0, 0xffu, 300.f);
      for (int i = OSH_FUSE_MAX_CELL_ENTRIES; i < OSH_FUSE_MAX_KEYS; ++i) {   // four to a cell; those of the full cell go to cell (0, 0)
        const int cx = i % 128, cy = (i / 128) % 128;
        const bool full = cx == 64 && cy == 64;
        t.add(full ? 0.5f : 5.f * cx + 0.5f, full ? 0.5f : 3.75f * cy + 0.5f, i % 8, (uint32_t)i);
      }
      const osh::FuseKeys k = t.bin(true);
      CHECK(t.most == OSH_FUSE_MAX_CELL_ENTRIES && t.T.n_keys == OSH_FUSE_MAX_KEYS);
      const Out o = run(t, k, {0.f, 0.f, 2.f}, axis, 0.1f, 2.f, mode);
      CHECK(o.g.stage == OSH_FUSE_SEARCHED && o.f.n_in == OSH_FUSE_MAX_CELL_ENTRIES && o.f.best_idx == 0 && o.f.best_dist == 64);
      t.add(320.f, 240.f, 0, 0u);   // one more in the full cell: the binning reports it and fills nothing
      t.bin(true);
      CHECK(t.most > OSH_FUSE_MAX_CELL_ENTRIES);
    }
    {   // OSH_FUSE_MAX_TARGETS targets of one keypoint on a 1 x 1 grid
      for (int n = 0; n < OSH_FUSE_MAX_TARGETS; ++n) {
        Target t(1, 1, 1, 3.f);
        t.add(100.f, 100.f, 0, (uint32_t)n);   // PosInGrid rounds: the centre of the image would be cell 1 of 1
        const osh::FuseKeys k = t.bin(false);
        const Out o = run(t, k, {-1.71875f, -1.09375f, 2.f}, axis, 0.1f, 4.f, mode);
        CHECK(o.g.stage == OSH_FUSE_SEARCHED && o.f.best_idx == 0 && o.f.best_dist == 8 * __builtin_popcount((unsigned)n));
      }
    }
  }
  // the conversions: what no int holds, and the cell numbers only the comparison with the grid matters for
  CHECK(osh::fuse_level(1.f, 0.f, 0.18f, 8) == 0 && osh::fuse_level(nan, 1.f, 0.18f, 8) == 0 && osh::fuse_level(0.f, 1.f, 0.18f, 8) == 0);
  CHECK(osh::fuse_level(1e30f, 1.f, 0.18f, 8) == 7 && osh::fuse_level(1.f, 1.f, 0.18f, 8) == 0);
  CHECK(osh::fuse_cell(nan) == -1 && osh::fuse_cell(-inf) == -1 && osh::fuse_cell(inf) == -1 && osh::fuse_cell(3.0e9f) == -1 && osh::fuse_cell(2.0e9f) == OSH_FUSE_MAX_CELLS && osh::fuse_cell(-0.f) == 0 && osh::fuse_cell(7.f) == 7);
  std::printf("fuse_check ok: %ld checks\n", checks);
  return 0;
}
