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
// A frame reads the pyramid its token names (the copy osh_orb_fast_detect left on the context) or brings its own.
#include "common.h"
#include "orb_brief.h"
#include "orb_fast_state.h"
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

struct BlurLevelDev {
  const unsigned char* src;    // first pixel of the packed level
  unsigned char* dst;          // of the blurred level
  int rows, cols;
  unsigned short w[8];         // w[0..6]
};
struct BlurTileDev { int level, tx, ty; };

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

struct BriefLevelDev { const unsigned char* blurred; int rows, cols; };
struct BriefView {
  int n;
  const BriefLevelDev* levels;     // of every frame of the call, frame after frame
  const int* level_index;          // [n] the keypoint's entry of `levels`
  const int* frame;                // [n] the keypoint's frame: its table
  const float2* xy;                // [n]
  const float* angle;              // [n]
  const signed char* pattern;      // [n_frames * 1024]
  unsigned long long* desc;        // [n * 4]
  float2* cos_sin;                 // [n]
};

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
  const BriefLevelDev L = v.levels[v.level_index[i]];
  const float2 p = v.xy[i];
  const BriefRot r = brief_rotation(v.angle[i]);
  const unsigned char* centre = L.blurred + (size_t)fast_cv_round(p.y) * L.cols + fast_cv_round(p.x);
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

// One frame's table, weights, keypoints and result arrays against the level sizes rows[] / cols[]
static int brief_validate_frame(int k, const osh_describe_frame& f, const osh_describe_result& r, int n_levels, const int* rows, const int* cols) {
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
  const int R = brief_reach(f.pattern);
  for (int i = 0; i < f.n; ++i) {
    const float x = f.xy[2 * i], y = f.xy[2 * i + 1];
    const int l = f.level[i];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(f.angle[i])) { set_error("osh_orb_describe: frame %d: keypoint %d is not finite", k, i); return OSH_ERR_INVALID; }
    if (l < 0 || l >= n_levels) { set_error("osh_orb_describe: frame %d: keypoint %d: level %d outside [0, %d)", k, i, l, n_levels); return OSH_ERR_INVALID; }
    // compared as floats first: a coordinate beyond the int range must not reach the conversion
    bool inside = x >= 0.f && y >= 0.f && x <= (float)OSH_FAST_MAX_SIDE && y <= (float)OSH_FAST_MAX_SIDE && rows[l] >= kBriefMinSide && cols[l] >= kBriefMinSide;
    if (inside) {
      const int cx = fast_cv_round(x), cy = fast_cv_round(y);
      inside = cx - R >= 0 && cx + R < cols[l] && cy - R >= 0 && cy + R < rows[l];
    }
    if (!inside) { set_error("osh_orb_describe: frame %d: keypoint %d: the %d-pixel square leaves level %d", k, i, 2 * R + 1, l); return OSH_ERR_INVALID; }
  }
  if (r.blurred)
    for (int l = 0; l < n_levels; ++l)
      if (rows[l] < kBriefMinSide || cols[l] < kBriefMinSide) { set_error("osh_orb_describe: frame %d: level %d has fewer than %d rows or columns: no blur", k, l, kBriefMinSide); return OSH_ERR_UNSUPPORTED; }
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_describe(osh_orb_ctx* c, int32_t n_frames, const osh_describe_frame* frames, const osh_describe_result* results) {
  PhaseClock clock;
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_describe: bad arguments"); return OSH_ERR_INVALID; }
  // frames that bring their pyramid first: their refusals need no context and no device
  bool any_token = false;
  size_t N = 0;
  for (int k = 0; k < n_frames; ++k) {
    const osh_describe_frame& f = frames[k];
    if (!f.pyramid) { any_token = true; continue; }
    OSH_TRY(fast_validate_pyramid("osh_orb_describe", k, f.n_levels, f.pyramid));
    int rows[OSH_STEREO_MAX_LEVELS], cols[OSH_STEREO_MAX_LEVELS];
    for (int l = 0; l < f.n_levels; ++l) { rows[l] = f.pyramid[l].rows; cols[l] = f.pyramid[l].cols; }
    OSH_TRY(brief_validate_frame(k, f, results[k], f.n_levels, rows, cols));
  }
  if (!c) { set_error("osh_orb_describe: no context"); return OSH_ERR_INVALID; }
  FastState* fs = any_token ? orb_state<FastState>(c, kOrbAttachFast) : nullptr;
  for (int k = 0; k < n_frames; ++k) {
    const osh_describe_frame& f = frames[k];
    if (f.pyramid) continue;
    const FastFrameHost* F = fast_resident_frame(fs, f.pyramid_token);
    if (!F) { set_error("osh_orb_describe: frame %d: the token names no frame of this context's last osh_orb_fast_detect", k); return OSH_ERR_INVALID; }
    int rows[OSH_STEREO_MAX_LEVELS], cols[OSH_STEREO_MAX_LEVELS];
    for (int l = 0; l < F->n_levels; ++l) { rows[l] = fs->levels[F->level0 + l].rows; cols[l] = fs->levels[F->level0 + l].cols; }
    OSH_TRY(brief_validate_frame(k, f, results[k], F->n_levels, rows, cols));
  }
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

  // levels of the call: a frame with a token points into the resident arena of the detector, the others into this call's upload;
  // the blurred arena packs all of them in this order
  struct Lv { bool resident; size_t off, blur_off; int rows, cols, frame; bool wanted; };
  std::vector<Lv> lv;
  std::vector<int> level0(n_frames), n_levels(n_frames);
  size_t img_bytes = 0, blur_bytes = 0;
  for (int k = 0; k < n_frames; ++k) {
    const osh_describe_frame& f = frames[k];
    level0[k] = (int)lv.size();
    const bool all = results[k].blurred != nullptr;
    if (f.pyramid) {
      n_levels[k] = f.n_levels;
      for (int l = 0; l < f.n_levels; ++l) {
        const size_t bytes = (size_t)f.pyramid[l].rows * f.pyramid[l].cols;
        lv.push_back({false, img_bytes, blur_bytes, f.pyramid[l].rows, f.pyramid[l].cols, k, all});
        img_bytes += bytes; blur_bytes += bytes;
      }
    } else {
      const FastFrameHost* F = fast_resident_frame(fs, f.pyramid_token);
      n_levels[k] = F->n_levels;
      for (int l = 0; l < F->n_levels; ++l) {
        const FastLevelHost& L = fs->levels[F->level0 + l];
        lv.push_back({true, (size_t)L.img_off, blur_bytes, L.rows, L.cols, k, all});
        blur_bytes += (size_t)L.rows * L.cols;
      }
    }
    for (int i = 0; i < f.n; ++i) lv[level0[k] + f.level[i]].wanted = true;
    if (img_bytes > (size_t)1 << 31 || blur_bytes > (size_t)1 << 32) { set_error("osh_orb_describe: batch too large"); return OSH_ERR_UNSUPPORTED; }
  }
  std::vector<BlurTileDev> tiles;
  for (size_t l = 0; l < lv.size(); ++l) {
    if (!lv[l].wanted) continue;
    const int nty = (lv[l].rows + kBlurTH - 1) / kBlurTH, ntx = (lv[l].cols + kBlurTW - 1) / kBlurTW;
    for (int ty = 0; ty < nty; ++ty) for (int tx = 0; tx < ntx; ++tx) tiles.push_back({(int)l, tx, ty});
  }

  Layout in, out;
  const auto s_blur = in.take<BlurLevelDev>(lv.size());
  const auto s_levels = in.take<BriefLevelDev>(lv.size());
  const auto s_tiles = in.take<BlurTileDev>(tiles.size());
  const auto s_index = in.take<int>(N);
  const auto s_frame = in.take<int>(N);
  const auto s_xy = in.take<float2>(N);
  const auto s_angle = in.take<float>(N);
  const auto s_pattern = in.take<signed char>((size_t)n_frames * 2 * kBriefPoints);
  const auto s_img = in.take<unsigned char>(img_bytes);
  const auto o_desc = out.take<unsigned long long>(N * 4);
  const auto o_cs = out.take<float2>(N);
  OSH_TRY(st->call.reserve(in, out));
  OSH_TRY(st->blurred.reserve(blur_bytes));
  char* h = st->call.host_in();
  const unsigned char* resident = fs ? fast_resident_images(fs) : nullptr;
  const unsigned char* uploaded = s_img.in(static_cast<const char*>(st->call.dev_in()));
  unsigned char* blurred = st->blurred.as<unsigned char>();
  uint16_t default_w[kBriefTaps];
  brief_gaussian_q8(kBriefTaps, 2.0, default_w);
  for (size_t l = 0; l < lv.size(); ++l) {
    BlurLevelDev& B = s_blur.in(h)[l];
    B.src = (lv[l].resident ? resident : uploaded) + lv[l].off; B.dst = blurred + lv[l].blur_off; B.rows = lv[l].rows; B.cols = lv[l].cols;
    const uint16_t* w = frames[lv[l].frame].blur_q8 ? frames[lv[l].frame].blur_q8 : default_w;
    for (int u = 0; u < kBriefTaps; ++u) B.w[u] = w[u];
    B.w[7] = 0;
    s_levels.in(h)[l] = {B.dst, lv[l].rows, lv[l].cols};
  }
  if (!tiles.empty()) std::memcpy(s_tiles.in(h), tiles.data(), sizeof(BlurTileDev) * tiles.size());
  std::vector<size_t> base(n_frames);
  size_t b = 0;
  for (int k = 0; k < n_frames; ++k) {
    const osh_describe_frame& f = frames[k];
    base[k] = b;
    if (f.n) { std::memcpy(s_xy.in(h) + b, f.xy, (size_t)f.n * 8); std::memcpy(s_angle.in(h) + b, f.angle, (size_t)f.n * 4); }
    for (int i = 0; i < f.n; ++i) { s_index.in(h)[b + i] = level0[k] + f.level[i]; s_frame.in(h)[b + i] = k; }
    b += (size_t)f.n;
    std::memcpy(s_pattern.in(h) + (size_t)k * 2 * kBriefPoints, f.pattern, 2 * kBriefPoints);
    if (f.pyramid) for (int l = 0; l < f.n_levels; ++l) pack_level(s_img.in(h) + lv[level0[k] + l].off, f.pyramid[l]);
  }
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));
  char* di = st->call.dev_in(); char* dout = st->call.dev_out();
  if (!tiles.empty()) hipLaunchKernelGGL(k_orb_blur, dim3((unsigned)tiles.size()), dim3(kBlurBlock), 0, s, s_blur.in(di), s_tiles.in(di));
  if (N) {
    BriefView v{};
    v.n = (int)N; v.levels = s_levels.in(di); v.level_index = s_index.in(di); v.frame = s_frame.in(di); v.xy = s_xy.in(di);
    v.angle = s_angle.in(di); v.pattern = s_pattern.in(di); v.desc = o_desc.in(dout); v.cos_sin = o_cs.in(dout);
    hipLaunchKernelGGL(k_orb_brief, dim3((unsigned)((N + kBriefBlock / 64 - 1) / (kBriefBlock / 64))), dim3(kBriefBlock), 0, s, v);
  }
  OSH_TRY(launch_check("ORB blur and descriptors"));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));   // synchronises
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_frames; ++k) {
    const size_t n = (size_t)frames[k].n;
    scatter(reinterpret_cast<unsigned long long*>(results[k].descriptors), o_desc, ho, base[k], n, 4);
    scatter(reinterpret_cast<float2*>(results[k].cos_sin), o_cs, ho, base[k], n);
    if (results[k].blurred && n_levels[k]) {
      const Lv& first = lv[level0[k]];
      const Lv& last = lv[level0[k] + n_levels[k] - 1];
      const size_t bytes = last.blur_off + (size_t)last.rows * last.cols - first.blur_off;
      OSH_HIP(hipMemcpyAsync(results[k].blurred, blurred + first.blur_off, bytes, hipMemcpyDeviceToHost, s));
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
