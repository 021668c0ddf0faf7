// orb_pyramid_device.hip -- ORBextractor::ComputePyramid (src/ORBextractor.cc:1170-1195) on MI355X (gfx950) for a batch of images:
// every level of every frame is resampled on the device from the level before it and stays there as the context's resident pyramid
// (orb_pyramid_set.h), under one token per frame, for osh_orb_fast_detect_resident, osh_orb_ic_angle and osh_orb_describe.  The
// statements are those of orb_pyramid.h; the kernels are integer only and the tap tables are input data computed on the host.
//
// osh_orb_pyramid_build:
//   the images are packed into pinned memory and uploaded as the level 0 of every frame (they lie one after another at the start of
//   the resident buffer, so it is one copy), together with the jobs and the tap tables (one pair per distinct (src, dst) geometry);
//   k_pyr_level    once per level l >= 1 over all frames that have it (grid y: the frame): a thread produces four horizontally
//                  adjacent pixels of one row from the two source rows and stores them as one dword.  Levels are packed at `cols`
//                  bytes per row, so a row starts at any byte: the groups are formed on the absolute address (the first group of a
//                  row holds the 1-4 pixels up to the next dword boundary), and a group that is cut by either end of its row is
//                  stored byte by byte.  No store crosses a row or is misaligned.
//   k_pyr_border   only when a frame asks for its levels: every level with `border` pixels around it by reflect-101 into an arena
//                  of its own (rows padded to dwords), one D2H copy, and the rows scattered into the caller's images.
// Level l waits for level l - 1 through the order of the stream: ordinary launches, no barrier across blocks.
// pyramid_build_from (orb_extract.h) is the body: osh_orb_pyramid_build and osh_orb_extract call it with the upload above, and
// osh_orb_extract_raw (orb_prepare_device.hip) with a device producer that writes level 0 on the stream before k_pyr_level.
#include "common.h"
#include "orb_extract.h"
#include "orb_pyramid_set.h"
#include "orb_pyramid.h"
#include "orb_stage.h"
#include <cmath>
#include <map>
#include <tuple>
#include <vector>

namespace osh {

constexpr int kPyrBlockX = 64, kPyrBlockY = 4;   // k_pyr_level: 64 groups of four pixels by 4 rows
constexpr int kPyrBorderBlock = 256;

struct PyrJobDev {
  long long src_off, dst_off;   // first pixel of the two levels in the resident buffer
  int src_rows, src_cols, dst_rows, dst_cols;
  int col_tap, row_tap;         // first entry of the level's tables in `taps`
  int halving;                  // the exact-halving path: no tables
  int groups;                   // dword groups a row can touch: (dst_cols + 6) / 4
};
struct PyrBorderJobDev {
  long long src_off, dst_off;   // the level in the resident buffer; the bordered level in the arena (dword aligned)
  int rows, cols, border, pitch;   // pitch: bytes per bordered row, a multiple of 4
};
struct PyrView {
  const PyrJobDev* jobs;
  const PyrBorderJobDev* border_jobs;
  const PyrTap* taps;
  unsigned char* images;        // the resident buffer
  unsigned char* bordered;
};

__global__ __launch_bounds__(kPyrBlockX * kPyrBlockY) void k_pyr_level(PyrView v, int job0) {
  const PyrJobDev& J = v.jobs[job0 + blockIdx.y];
  const int tiles_x = (J.groups + kPyrBlockX - 1) / kPyrBlockX;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y = ty * kPyrBlockY + threadIdx.y, g = tx * kPyrBlockX + threadIdx.x;
  if (y >= J.dst_rows) return;
  const long long row = J.dst_off + (long long)y * J.dst_cols;   // byte offset of the row; the buffer itself is 256-byte aligned
  const int lead = (int)(row & 3);
  const int x0 = 4 * g - lead;                                   // row + x0 is a multiple of 4
  if (x0 >= J.dst_cols) return;
  const unsigned char* src = v.images + J.src_off;
  const unsigned char *r0, *r1;
  int b0 = 0, b1 = 0;
  if (J.halving) {
    r0 = src + (size_t)(2 * y) * J.src_cols; r1 = r0 + J.src_cols;
  } else {
    const PyrTap ry = v.taps[J.row_tap + y];
    r0 = src + (size_t)ry.s0 * J.src_cols; r1 = src + (size_t)ry.s1 * J.src_cols;
    b0 = ry.w0; b1 = ry.w1;
  }
  unsigned px[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int x = x0 + i;
    px[i] = 0;
    if (x >= 0 && x < J.dst_cols) px[i] = J.halving ? pyr_half_pixel(r0, r1, x) : pyr_pixel(r0, r1, v.taps[J.col_tap + x], b0, b1);
  }
  unsigned char* dst = v.images + row + x0;
  if (x0 >= 0 && x0 + 3 < J.dst_cols) {
    *reinterpret_cast<unsigned*>(dst) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x0 + i >= 0 && x0 + i < J.dst_cols) dst[i] = (unsigned char)px[i];
  }
}

// One dword of a bordered level per thread; the padding at the end of a row is written as zeros
__global__ __launch_bounds__(kPyrBorderBlock) void k_pyr_border(PyrView v) {
  const PyrBorderJobDev& J = v.border_jobs[blockIdx.y];
  const int words = J.pitch / 4, width = J.cols + 2 * J.border;
  const long long idx = (long long)blockIdx.x * kPyrBorderBlock + threadIdx.x;
  if (idx >= (long long)words * (J.rows + 2 * J.border)) return;
  const int yb = (int)(idx / words), xw = (int)(idx - (long long)yb * words);
  const unsigned char* src = v.images + J.src_off + (size_t)pyr_reflect101(yb - J.border, J.rows) * J.cols;
  unsigned word = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int xb = 4 * xw + i;
    if (xb < width) word |= (unsigned)src[pyr_reflect101(xb - J.border, J.cols)] << (8 * i);
  }
  *reinterpret_cast<unsigned*>(v.bordered + J.dst_off + (size_t)yb * J.pitch + 4 * (size_t)xw) = word;
}

struct PyrFrameHost { int rows[OSH_STEREO_MAX_LEVELS], cols[OSH_STEREO_MAX_LEVELS]; };

// device_level0: the image brings no data (a device producer makes level 0), its size is checked all the same
static int pyramid_validate(int k, const osh_pyramid_frame& f, const osh_pyramid_result& r, PyrFrameHost& sz, bool device_level0) {
  const char* entry = "osh_orb_pyramid_build";
  osh_stereo_image im = f.image;
  if (device_level0) { im.data = reinterpret_cast<const uint8_t*>(&im); im.stride = im.cols; }   // not read: only NULL is refused
  OSH_TRY(fast_validate_pyramid(entry, k, 1, &im));
  if (f.n_levels < 1 || f.n_levels > OSH_STEREO_MAX_LEVELS) { set_error("%s: frame %d: n_levels %d outside [1, %d]", entry, k, f.n_levels, OSH_STEREO_MAX_LEVELS); return OSH_ERR_INVALID; }
  if (!f.inv_scale) { set_error("%s: frame %d: NULL inv_scale", entry, k); return OSH_ERR_INVALID; }
  if (r.border < 0) { set_error("%s: frame %d: negative border", entry, k); return OSH_ERR_INVALID; }
  for (int l = 0; l < f.n_levels; ++l) {
    const float inv = f.inv_scale[l];
    if (!std::isfinite(inv) || !(inv > 0.f)) { set_error("%s: frame %d: inv_scale[%d] is not a finite positive number", entry, k, l); return OSH_ERR_INVALID; }
    sz.rows[l] = pyr_level_size(f.image.rows, inv); sz.cols[l] = pyr_level_size(f.image.cols, inv);
    if (sz.rows[l] <= 0 || sz.cols[l] <= 0) { set_error("%s: frame %d: level %d rounds to 0 pixels in a direction", entry, k, l); return OSH_ERR_INVALID; }
    if (l == 0 && (sz.rows[0] != f.image.rows || sz.cols[0] != f.image.cols)) { set_error("%s: frame %d: level 0 is %d x %d, not the image's %d x %d", entry, k, sz.rows[0], sz.cols[0], f.image.rows, f.image.cols); return OSH_ERR_INVALID; }
    if (sz.rows[l] > OSH_FAST_MAX_SIDE || sz.cols[l] > OSH_FAST_MAX_SIDE) { set_error("%s: frame %d: level %d exceeds %d pixels in one direction", entry, k, l, OSH_FAST_MAX_SIDE); return OSH_ERR_UNSUPPORTED; }
    if (r.levels) {
      const osh_pyramid_image& o = r.levels[l];
      if (!o.data || o.rows != sz.rows[l] || o.cols != sz.cols[l] || o.stride < (int64_t)sz.cols[l] + 2 * (int64_t)r.border) {
        set_error("%s: frame %d: levels[%d] is NULL, is not %d x %d or has stride < cols + 2 border", entry, k, l, sz.rows[l], sz.cols[l]); return OSH_ERR_INVALID;
      }
    }
  }
  return OSH_OK;
}

// The body of osh_orb_pyramid_build: the sizing, the tables, the jobs, the launch of the upper levels, the bordered download and the
// commit.  Level 0 comes from the host images (producer == nullptr: packed and uploaded) or from a device producer that runs on the
// stream before k_pyr_level (orb_extract.h).
int pyramid_build_from(osh_orb_ctx* c, int32_t n_frames, const osh_pyramid_frame* frames, osh_pyramid_result* results, const Level0Producer* producer) {
  PhaseClock clock;
  const char* entry = "osh_orb_pyramid_build";
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  std::vector<PyrFrameHost> sz((size_t)n_frames);
  for (int k = 0; k < n_frames; ++k) OSH_TRY(pyramid_validate(k, frames[k], results[k], sz[k], producer != nullptr));   // a refusal needs no context and no device
  if (!c) { set_error("%s: no context", entry); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  if (n_frames > 65535) { set_error("%s: more than 65535 frames in one call", entry); return OSH_ERR_UNSUPPORTED; }

  // the resident buffer: the level 0 of every frame first (one upload), then the other levels frame after frame
  std::vector<FastFrameHost> fh((size_t)n_frames);
  std::vector<FastLevelHost> lh;
  size_t bytes = 0;
  for (int k = 0; k < n_frames; ++k) {
    fh[k] = {(int)lh.size(), frames[k].n_levels, 0, 0};
    for (int l = 0; l < frames[k].n_levels; ++l) lh.push_back({0, sz[k].rows[l], sz[k].cols[l], 0, 0});
    lh[fh[k].level0].img_off = (long long)bytes;
    bytes += (size_t)sz[k].rows[0] * sz[k].cols[0];
  }
  const size_t img0_bytes = bytes;
  for (int k = 0; k < n_frames; ++k)
    for (int l = 1; l < frames[k].n_levels; ++l) {
      lh[fh[k].level0 + l].img_off = (long long)bytes;
      bytes += (size_t)sz[k].rows[l] * sz[k].cols[l];
    }
  if (bytes > (size_t)1 << 31) { set_error("%s: batch too large", entry); return OSH_ERR_UNSUPPORTED; }

  // jobs level by level, the tables once per geometry
  std::vector<PyrJobDev> jobs;
  std::vector<PyrTap> taps;
  std::map<std::tuple<int, int, bool>, int> table_at;
  auto table = [&](int src, int dst, bool rows) {
    const auto key = std::make_tuple(src, dst, rows);
    const auto it = table_at.find(key);
    if (it != table_at.end()) return it->second;
    const int at = (int)taps.size();
    taps.resize(taps.size() + (size_t)dst);
    pyr_axis_table(src, dst, rows, taps.data() + at);
    table_at.emplace(key, at);
    return at;
  };
  int level_job0[OSH_STEREO_MAX_LEVELS + 1] = {0}, level_tiles[OSH_STEREO_MAX_LEVELS] = {0};
  for (int l = 1; l < OSH_STEREO_MAX_LEVELS; ++l) {
    level_job0[l] = (int)jobs.size();
    for (int k = 0; k < n_frames; ++k) {
      if (frames[k].n_levels <= l) continue;
      const FastLevelHost& S = lh[fh[k].level0 + l - 1];
      const FastLevelHost& D = lh[fh[k].level0 + l];
      PyrJobDev J{S.img_off, D.img_off, S.rows, S.cols, D.rows, D.cols, 0, 0, pyr_is_halving(S.rows, S.cols, D.rows, D.cols) ? 1 : 0, (D.cols + 6) / 4};
      if (!J.halving) { J.col_tap = table(S.cols, D.cols, false); J.row_tap = table(S.rows, D.rows, true); }
      jobs.push_back(J);
      const int tiles = ((J.groups + kPyrBlockX - 1) / kPyrBlockX) * ((D.rows + kPyrBlockY - 1) / kPyrBlockY);
      level_tiles[l] = std::max(level_tiles[l], tiles);
    }
  }
  level_job0[OSH_STEREO_MAX_LEVELS] = (int)jobs.size();

  // the bordered levels of the frames that ask for them
  std::vector<PyrBorderJobDev> bjobs;
  struct Want { int frame, level; };
  std::vector<Want> want;
  size_t bordered_bytes = 0;
  long long border_blocks = 0;
  for (int k = 0; k < n_frames; ++k) {
    if (!results[k].levels) continue;
    const int b = results[k].border;
    for (int l = 0; l < frames[k].n_levels; ++l) {
      const FastLevelHost& L = lh[fh[k].level0 + l];
      const int pitch = (L.cols + 2 * b + 3) & ~3;
      const size_t rows = (size_t)L.rows + 2 * (size_t)b;
      bjobs.push_back({L.img_off, (long long)bordered_bytes, L.rows, L.cols, b, pitch});
      want.push_back({k, l});
      border_blocks = std::max(border_blocks, (long long)(((size_t)(pitch / 4) * rows + kPyrBorderBlock - 1) / kPyrBorderBlock));
      bordered_bytes += ((size_t)pitch * rows + 255) & ~(size_t)255;
      if (bordered_bytes > (size_t)1 << 31 || b > OSH_FAST_MAX_SIDE) { set_error("%s: download too large", entry); return OSH_ERR_UNSUPPORTED; }
    }
  }
  if (bjobs.size() > 65535) { set_error("%s: more than 65535 levels to download in one call", entry); return OSH_ERR_UNSUPPORTED; }

  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  if (producer) OSH_TRY(producer->check(device));   // its refusals that need the context's device: the resident pyramid stays
  FastState* st = orb_state<FastState>(c, kOrbAttachFast);
  clock.profiling = orb_profiling(c);
  st->pyramid.invalidate();   // the resident pyramid is about to be replaced

  Layout in, out;
  const auto s_jobs = in.take<PyrJobDev>(jobs.size());
  const auto s_bjobs = in.take<PyrBorderJobDev>(bjobs.size());
  const auto s_taps = in.take<PyrTap>(taps.size());
  out.take<int>(1);   // nothing comes back through this staging; an empty region has no pinned buffer
  OSH_TRY(st->pyr_call.reserve(in, out));
  OSH_TRY(st->pyramid.buffer.reserve(bytes));
  unsigned char* hi = producer ? nullptr : static_cast<unsigned char*>(st->pyramid.h_images.reserve(img0_bytes));
  if (!producer && !hi) { set_error("%s: pinned allocation of %zu bytes failed", entry, img0_bytes); return OSH_ERR_DEVICE; }
  if (bordered_bytes) {
    OSH_TRY(st->bordered.reserve(bordered_bytes));
    if (!st->h_bordered.reserve(bordered_bytes)) { set_error("%s: pinned allocation of %zu bytes failed", entry, bordered_bytes); return OSH_ERR_DEVICE; }
  }
  char* h = st->pyr_call.host_in();
  if (!jobs.empty()) std::memcpy(s_jobs.in(h), jobs.data(), sizeof(PyrJobDev) * jobs.size());
  if (!bjobs.empty()) std::memcpy(s_bjobs.in(h), bjobs.data(), sizeof(PyrBorderJobDev) * bjobs.size());
  if (!taps.empty()) std::memcpy(s_taps.in(h), taps.data(), sizeof(PyrTap) * taps.size());
  for (int k = 0; !producer && k < n_frames; ++k) pack_level(hi + lh[fh[k].level0].img_off, frames[k].image);
  clock.mark();
  OSH_TRY(st->pyr_call.upload(s));
  if (producer) {
    std::vector<long long> level0_off((size_t)n_frames);
    for (int k = 0; k < n_frames; ++k) level0_off[k] = lh[fh[k].level0].img_off;
    OSH_TRY(producer->produce(s, st->pyramid.buffer.as<unsigned char>(), level0_off));
  } else {
    OSH_HIP(hipMemcpyAsync(st->pyramid.buffer.p, hi, img0_bytes, hipMemcpyHostToDevice, s));
  }
  OSH_TRY(clock.mark_synced(s));

  PyrView v{};
  char* di = st->pyr_call.dev_in();
  v.jobs = s_jobs.in(di); v.border_jobs = s_bjobs.in(di); v.taps = s_taps.in(di);
  v.images = st->pyramid.buffer.as<unsigned char>(); v.bordered = st->bordered.as<unsigned char>();
  for (int l = 1; l < OSH_STEREO_MAX_LEVELS; ++l) {
    const int n = level_job0[l + 1] - level_job0[l];
    if (n) hipLaunchKernelGGL(k_pyr_level, dim3((unsigned)level_tiles[l], (unsigned)n), dim3(kPyrBlockX, kPyrBlockY), 0, s, v, level_job0[l]);
  }
  if (!bjobs.empty()) hipLaunchKernelGGL(k_pyr_border, dim3((unsigned)border_blocks, (unsigned)bjobs.size()), dim3(kPyrBorderBlock), 0, s, v);
  OSH_TRY(launch_check("pyramid"));
  OSH_HIP(hipStreamSynchronize(s));   // the staging buffers are free again when the call returns
  clock.mark();
  if (bordered_bytes) {
    OSH_HIP(hipMemcpyAsync(st->h_bordered.p, st->bordered.p, bordered_bytes, hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
    const unsigned char* hb = static_cast<const unsigned char*>(st->h_bordered.p);
    for (size_t j = 0; j < bjobs.size(); ++j) {
      const PyrBorderJobDev& J = bjobs[j];
      const osh_pyramid_image& o = results[want[j].frame].levels[want[j].level];
      for (int y = -J.border; y < J.rows + J.border; ++y)
        std::memcpy(o.data + (long long)y * o.stride - J.border, hb + J.dst_off + (size_t)(y + J.border) * J.pitch, (size_t)J.cols + 2 * (size_t)J.border);
    }
  }
  const uint64_t token0 = st->pyramid.commit(std::move(fh), std::move(lh));
  for (int k = 0; k < n_frames; ++k) {
    results[k].pyramid_token = token0 + (uint64_t)k;
    for (int l = 0; l < frames[k].n_levels; ++l) {
      if (results[k].level_rows) results[k].level_rows[l] = sz[k].rows[l];
      if (results[k].level_cols) results[k].level_cols[l] = sz[k].cols[l];
    }
  }
  clock.mark();
  clock.store(st->ms_pyr);
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_pyramid_build(osh_orb_ctx* c, int32_t n_frames, const osh_pyramid_frame* frames, osh_pyramid_result* results) {
  return pyramid_build_from(c, n_frames, frames, results, nullptr);
}

extern "C" int osh_orb_pyramid_get_times(osh_orb_ctx* c, double ms[4]) {
  if (!c || !ms) { set_error("osh_orb_pyramid_get_times: bad arguments"); return OSH_ERR_INVALID; }
  std::memcpy(ms, orb_state<FastState>(c, kOrbAttachFast)->ms_pyr, sizeof(double) * 4);
  return OSH_OK;
}
