// orb_brief_device.hip -- what ORBextractor::operator() (src/ORBextractor.cc:1123-1165) runs per level after ComputeKeyPointsOctTree,
// on MI355X (gfx950) for a batch of pyramids: the 7x7 blur of every level that holds a keypoint and the 256 rotated comparisons of
// every keypoint.  The statements are those of orb_brief.h.
//
// osh_orb_describe:
//   k_orb_blur    one block per 64 x 16 output tile of a level: the tile with its 3-pixel halo into LDS through the reflected
//                 indices (70 x 22 bytes), the horizontal pass into 16-bit LDS (64 x 22), the vertical pass, bytes into the blurred
//                 arena, which has the layout of the packed pyramid.
//   k_orb_brief   one wavefront per keypoint, four per block, each with its frame's table in LDS (the keypoints of a block may belong
//                 to frames with different tables): lane t evaluates pairs t, 64 + t, 128 + t, 192 + t; each of the four ballots
//                 is eight consecutive descriptor bytes.  No atomic.  The samples are gathered from the blurred level in global
//                 memory; staging the keypoint's window in LDS first was measured slower.
// A frame reads the pyramid its token names (the context's resident pyramid) or brings its own: orb_pyramid_set.h.
#include "common.h"
#include "orb_brief.h"
#include "orb_extract.h"
#include "orb_pyramid_set.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

constexpr int kBlurTW = 64, kBlurTH = 16;            // output tile: a wavefront per row, four rows per wavefront
constexpr int kBlurBlock = 256;
constexpr int kBlurInW = kBlurTW + 2 * kBriefHalo;   // 70
constexpr int kBlurInH = kBlurTH + 2 * kBriefHalo;   // 22
// LDS pitches.  Every wavefront access of the two passes touches ONE row: 64 consecutive bytes of sh_img (16 dwords, four lanes
// share a dword: a broadcast) or 64 consecutive 16-bit values of sh_h (32 dwords).  ds_read_u8 / u16 and every ds_write bank by
// (address / 4) % 32 within a 32-lane half, so a half sees at most 16 distinct consecutive dwords: conflict-free at any pitch.
// The pitches only keep the rows dword-aligned.
constexpr int kBlurImgPitch = 72;
constexpr int kBlurHPitch = kBlurTW;
constexpr int kBriefBlock = 256;                     // k_orb_brief: four keypoints

__global__ __launch_bounds__(kBlurBlock) void k_orb_blur(const BlurLevelDev* levels, const BlurTileDev* tiles) {
  __shared__ unsigned char sh_img[kBlurInH * kBlurImgPitch];
  __shared__ unsigned short sh_h[kBlurInH * kBlurHPitch];
  const BlurTileDev t = tiles[blockIdx.x];
  const BlurLevelDev& L = levels[t.level];
  const int rows = L.rows, cols = L.cols, x0 = t.tx * kBlurTW, y0 = t.ty * kBlurTH, tid = threadIdx.x;
  int w[kBriefTaps];
#pragma unroll
  for (int k = 0; k < kBriefTaps; ++k) w[k] = L.w[k];
  // the outputs of the tile need columns up to cols + 2 and rows up to rows + 2; what lies further feeds nothing and is read
  // from the last needed index, so that the reflection stays inside its domain
  for (int k = tid; k < kBlurInH * kBlurInW; k += kBlurBlock) {
    const int iy = k / kBlurInW, ix = k - iy * kBlurInW;
    const int gy = brief_reflect101(min(y0 - kBriefHalo + iy, rows - 1 + kBriefHalo), rows);
    const int gx = brief_reflect101(min(x0 - kBriefHalo + ix, cols - 1 + kBriefHalo), cols);
    sh_img[iy * kBlurImgPitch + ix] = L.src[(size_t)gy * cols + gx];
  }
  __syncthreads();
  const int lx = tid & 63, wave = tid >> 6;
  for (int iy = wave; iy < kBlurInH; iy += kBlurBlock / 64) {
    const unsigned char* p = &sh_img[iy * kBlurImgPitch + lx];
    int acc = 0;
#pragma unroll
    for (int u = 0; u < kBriefTaps; ++u) acc += w[u] * p[u];
    sh_h[iy * kBlurHPitch + lx] = (unsigned short)acc;
  }
  __syncthreads();
  const int gx = x0 + lx;
  for (int ly = wave; ly < kBlurTH; ly += kBlurBlock / 64) {
    const int gy = y0 + ly;
    int acc = 0;
#pragma unroll
    for (int v = 0; v < kBriefTaps; ++v) acc += w[v] * sh_h[(ly + v) * kBlurHPitch + lx];
    if (gx < cols && gy < rows) L.dst[(size_t)gy * cols + gx] = brief_blur_round(acc);
  }
}

__global__ __launch_bounds__(kBriefBlock) void k_orb_brief(BriefView v) {
  // the tables of the block's four keypoints; neighbours of one frame read the same bytes again, from L2
  __shared__ __attribute__((aligned(16))) signed char sh_pattern[kBriefBlock / 64][2 * kBriefPoints];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kBriefBlock / 64) + wave;
  const bool live = i < v.n;
  if (live) {
    const int4* src = reinterpret_cast<const int4*>(v.pattern + (size_t)v.frame[i] * 2 * kBriefPoints);
    reinterpret_cast<int4*>(sh_pattern[wave])[lane] = src[lane];   // 64 lanes x 16 bytes
  }
  __syncthreads();
  if (!live) return;
  const PyramidLevelDev L = v.levels[v.level_index[i]];
  const float2 p = v.xy[i];
  const BriefRot r = brief_rotation(v.angle[i]);
  const unsigned char* centre = L.data + (size_t)fast_cv_round(p.y) * L.cols + fast_cv_round(p.x);
  unsigned long long bits[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) bits[q] = __ballot(brief_pair(centre, L.cols, r, sh_pattern[wave], 64 * q + lane));
  if (lane < 4) v.desc[(size_t)i * 4 + lane] = lane == 0 ? bits[0] : lane == 1 ? bits[1] : lane == 2 ? bits[2] : bits[3];
  if (lane == 0) v.cos_sin[i] = make_float2(r.a, r.b);
}

struct BriefState {
  StagedCall call;       // [levels | tiles | keypoints | tables | pyramids brought along] in, [descriptors | cos_sin] out
  DevBuf blurred;        // the blurred levels of the call, packed like the pyramid
  double ms[4] = {0, 0, 0, 0};
};

// One frame's table, weights, keypoints and result arrays against its levels
static int brief_validate_frame(int k, const osh_describe_frame& f, const osh_describe_result& r, int n_levels, const PyramidLevel* lv) {
  if (f.n < 0) { set_error("osh_orb_describe: frame %d: negative keypoint count", k); return OSH_ERR_INVALID; }
  if (f.n && (!f.xy || !f.level || !f.angle)) { set_error("osh_orb_describe: frame %d: NULL keypoint array with n = %d", k, f.n); return OSH_ERR_INVALID; }
  if (f.n && !r.descriptors) { set_error("osh_orb_describe: frame %d: NULL descriptors with n = %d", k, f.n); return OSH_ERR_INVALID; }
  if (!f.pattern) { set_error("osh_orb_describe: frame %d: NULL pattern", k); return OSH_ERR_INVALID; }
  for (int i = 0; i < 2 * kBriefPoints; ++i)
    if (f.pattern[i] < -kBriefMaxCoord || f.pattern[i] > kBriefMaxCoord) { set_error("osh_orb_describe: frame %d: table point %d outside [-%d, %d]", k, i / 2, kBriefMaxCoord, kBriefMaxCoord); return OSH_ERR_INVALID; }
  if (f.blur_q8) {
    int sum = 0;
    for (int u = 0; u < kBriefTaps; ++u) sum += f.blur_q8[u];
    if (sum != 256) { set_error("osh_orb_describe: frame %d: the blur weights sum to %d, not 256", k, sum); return OSH_ERR_INVALID; }
  }
  bool angles_finite = true;   // the angles are this entry's alone: a pass of their own, without an exit inside it (no branch per keypoint)
  for (int i = 0; i < f.n; ++i) angles_finite &= std::isfinite(f.angle[i]);
  for (int i = 0; !angles_finite; ++i)
    if (!std::isfinite(f.angle[i])) { set_error("osh_orb_describe: frame %d: keypoint %d is not finite", k, i); return OSH_ERR_INVALID; }
  // a level without a blur holds no keypoint, whatever the table's reach: the keypoints see it as empty
  PyramidLevel blurred[OSH_STEREO_MAX_LEVELS];
  int no_blur = -1;
  for (int l = n_levels - 1; l >= 0; --l) {
    blurred[l] = lv[l];
    if (lv[l].rows < kBriefMinSide || lv[l].cols < kBriefMinSide) { blurred[l].rows = blurred[l].cols = 0; no_blur = l; }
  }
  OSH_TRY(validate_keypoints("osh_orb_describe", k, f.n, f.xy, f.level, n_levels, blurred, brief_reach(f.pattern), "square"));
  if (r.blurred && no_blur >= 0) { set_error("osh_orb_describe: frame %d: level %d has fewer than %d rows or columns: no blur", k, no_blur, kBriefMinSide); return OSH_ERR_UNSUPPORTED; }
  return OSH_OK;
}

BlurLevelDev blur_level(const unsigned char* src, unsigned char* dst, int rows, int cols, const uint16_t* w) {
  uint16_t default_w[kBriefTaps];
  if (!w) { brief_gaussian_q8(kBriefTaps, 2.0, default_w); w = default_w; }
  BlurLevelDev B{src, dst, rows, cols, {0, 0, 0, 0, 0, 0, 0, 0}};
  for (int u = 0; u < kBriefTaps; ++u) B.w[u] = w[u];
  return B;
}

void blur_tiles(int l, int rows, int cols, std::vector<BlurTileDev>& tiles) {
  const int nty = (rows + kBlurTH - 1) / kBlurTH, ntx = (cols + kBlurTW - 1) / kBlurTW;
  for (int ty = 0; ty < nty; ++ty) for (int tx = 0; tx < ntx; ++tx) tiles.push_back({l, tx, ty});
}

unsigned char* brief_blurred(osh_orb_ctx* c, size_t bytes) {
  BriefState* st = orb_state<BriefState>(c, kOrbAttachBrief);
  return st->blurred.reserve(bytes) == OSH_OK ? st->blurred.as<unsigned char>() : nullptr;
}

int brief_launch(hipStream_t s, size_t n_tiles, const BlurLevelDev* blur, const BlurTileDev* tiles, const BriefView& v) {
  if (n_tiles) hipLaunchKernelGGL(k_orb_blur, dim3((unsigned)n_tiles), dim3(kBlurBlock), 0, s, blur, tiles);
  if (v.n) hipLaunchKernelGGL(k_orb_brief, dim3((unsigned)((v.n + kBriefBlock / 64 - 1) / (kBriefBlock / 64))), dim3(kBriefBlock), 0, s, v);
  return launch_check("ORB blur and descriptors");
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_describe(osh_orb_ctx* c, int32_t n_frames, const osh_describe_frame* frames, const osh_describe_result* results) {
  PhaseClock clock;
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_describe: bad arguments"); return OSH_ERR_INVALID; }
  PyramidLevels<osh_describe_frame> pl{"osh_orb_describe", n_frames, frames};
  const auto frame_ok = [&](int k, int n_levels, const PyramidLevel* lv) { return brief_validate_frame(k, frames[k], results[k], n_levels, lv); };
  OSH_TRY(pl.check_brought(frame_ok));
  if (!c) { set_error("osh_orb_describe: no context"); return OSH_ERR_INVALID; }
  const ResidentPyramid* rp = pl.any_token ? &orb_state<FastState>(c, kOrbAttachFast)->pyramid : nullptr;
  OSH_TRY(pl.check_tokens(rp, frame_ok));
  size_t N = 0;
  for (int k = 0; k < n_frames; ++k) N += (size_t)frames[k].n;
  if (N > (size_t)1 << 24) { set_error("osh_orb_describe: more than 2^24 keypoints in one call"); return OSH_ERR_UNSUPPORTED; }
  bool any_blurred = false;
  for (int k = 0; k < n_frames; ++k) any_blurred |= results[k].blurred != nullptr;
  if (N == 0 && !any_blurred) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  BriefState* st = orb_state<BriefState>(c, kOrbAttachBrief);
  clock.profiling = orb_profiling(c);

  // the blurred arena packs the levels of the call in the order of the list; a level is blurred when it holds a keypoint or the
  // frame asks for its blurred levels
  OSH_TRY(pl.list(rp));
  const auto& lv = pl.lv;
  struct Blur { size_t off; int frame; bool wanted; };
  std::vector<Blur> blur(lv.size());
  size_t blur_bytes = 0;
  for (int k = 0; k < n_frames; ++k) {
    for (int l = pl.level0[k]; l < pl.level0[k] + pl.n_levels[k]; ++l) {
      blur[l] = {blur_bytes, k, results[k].blurred != nullptr};
      blur_bytes += (size_t)lv[l].rows * lv[l].cols;
    }
    for (int i = 0; i < frames[k].n; ++i) blur[pl.level0[k] + frames[k].level[i]].wanted = true;
    if (blur_bytes > (size_t)1 << 32) { set_error("osh_orb_describe: batch too large"); return OSH_ERR_UNSUPPORTED; }
  }
  std::vector<BlurTileDev> tiles;
  for (size_t l = 0; l < lv.size(); ++l)
    if (blur[l].wanted) blur_tiles((int)l, lv[l].rows, lv[l].cols, tiles);

  Layout in, out;
  const auto s_blur = in.take<BlurLevelDev>(lv.size());
  const auto s_levels = in.take<PyramidLevelDev>(lv.size());
  const auto s_tiles = in.take<BlurTileDev>(tiles.size());
  const auto s_index = in.take<int>(N);
  const auto s_frame = in.take<int>(N);
  const auto s_xy = in.take<float2>(N);
  const auto s_angle = in.take<float>(N);
  const auto s_pattern = in.take<signed char>((size_t)n_frames * 2 * kBriefPoints);
  const auto s_img = in.take<unsigned char>(pl.img_bytes);
  const auto o_desc = out.take<unsigned long long>(N * 4);
  const auto o_cs = out.take<float2>(N);
  OSH_TRY(st->call.reserve(in, out));
  OSH_TRY(st->blurred.reserve(blur_bytes));
  char* h = st->call.host_in();
  const unsigned char* resident = rp ? rp->images() : nullptr;
  const unsigned char* uploaded = s_img.in(static_cast<const char*>(st->call.dev_in()));
  unsigned char* blurred = st->blurred.as<unsigned char>();
  for (size_t l = 0; l < lv.size(); ++l) {
    const BlurLevelDev B = blur_level(pl.data(l, resident, uploaded), blurred + blur[l].off, lv[l].rows, lv[l].cols, frames[blur[l].frame].blur_q8);
    s_blur.in(h)[l] = B;
    s_levels.in(h)[l] = {B.dst, lv[l].rows, lv[l].cols};
  }
  if (!tiles.empty()) std::memcpy(s_tiles.in(h), tiles.data(), sizeof(BlurTileDev) * tiles.size());
  pl.index(s_index.in(h));
  pl.stage(s_img.in(h));
  std::vector<size_t> base(n_frames);
  size_t b = 0;
  for (int k = 0; k < n_frames; ++k) {
    const osh_describe_frame& f = frames[k];
    base[k] = b;
    if (f.n) { std::memcpy(s_xy.in(h) + b, f.xy, (size_t)f.n * 8); std::memcpy(s_angle.in(h) + b, f.angle, (size_t)f.n * 4); }
    std::fill_n(s_frame.in(h) + b, f.n, k);
    b += (size_t)f.n;
    std::memcpy(s_pattern.in(h) + (size_t)k * 2 * kBriefPoints, f.pattern, 2 * kBriefPoints);
  }
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));
  char* di = st->call.dev_in(); char* dout = st->call.dev_out();
  BriefView v{};
  v.n = (int)N; v.levels = s_levels.in(di); v.level_index = s_index.in(di); v.frame = s_frame.in(di); v.xy = s_xy.in(di);
  v.angle = s_angle.in(di); v.pattern = s_pattern.in(di); v.desc = o_desc.in(dout); v.cos_sin = o_cs.in(dout);
  OSH_TRY(brief_launch(s, tiles.size(), s_blur.in(di), s_tiles.in(di), v));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));   // synchronises
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_frames; ++k) {
    const size_t n = (size_t)frames[k].n;
    scatter(reinterpret_cast<unsigned long long*>(results[k].descriptors), o_desc, ho, base[k], n, 4);
    scatter(reinterpret_cast<float2*>(results[k].cos_sin), o_cs, ho, base[k], n);
    if (results[k].blurred && pl.n_levels[k]) {
      const size_t first = blur[pl.level0[k]].off, last = (size_t)pl.level0[k] + pl.n_levels[k] - 1;
      const size_t bytes = blur[last].off + (size_t)lv[last].rows * lv[last].cols - first;
      OSH_HIP(hipMemcpyAsync(results[k].blurred, blurred + first, bytes, hipMemcpyDeviceToHost, s));
      OSH_HIP(hipStreamSynchronize(s));
    }
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_describe_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<BriefState>("osh_orb_describe_get_times", c, kOrbAttachBrief, ms);
}
