// orb_extract_device.hip -- ORBextractor::operator() (src/ORBextractor.cc:1086-1168) for a batch of images in ONE call on MI355X
// (gfx950): osh_orb_extract.  The image goes up, keypoints and descriptors come back; between the detector and the descriptors no
// keypoint array crosses to the host.  The stages are the existing ones, each through its device-resident form (orb_extract.h):
//   osh_orb_pyramid_build          the levels, which become the context's resident pyramid with one token per frame;
//   fast_emit_resident             k_fast_cells, k_fast_scan, k_fast_emit on the resident levels; the cell offsets come down (they
//                                  size the emit buffer and say where every level's candidates are), the candidates stay;
//   octree_run                     k_octree, one workgroup per (frame, level) list, on the candidates where k_fast_emit left them; the
//                                  kept counts come down (they size what follows), the kept indices stay;
//   k_extract_gather               one wavefront per list: the kept candidates in level-then-list order with minBorder added (:880-890);
//   ic_angle_launch, brief_launch  k_ic_angle, k_orb_blur on the levels that hold a keypoint, k_orb_brief, all reading the gathered keypoints.
// Uploads besides the image: the plans of the stages (cells, lists, levels, tiles, tables).  One download at the end.
// A caller of extract_from may hang a tail behind brief_launch (ExtractTail of orb_extract.h): it chooses the order in which the frames'
// keypoints are laid out, adds its sections to the call's three layouts, launches on the same stream and reads its outputs from the
// same download.  osh_orb_extract_stereo (stereo_device.hip) does, with the stereo match; without a tail nothing changes.
// extract_from (orb_extract.h) is the body; osh_orb_extract_raw (orb_prepare_device.hip) calls it with a device producer of level 0.
#include "common.h"
#include "orb_brief.h"
#include "orb_extract.h"
#include "orb_fast.h"
#include "orb_octree.h"
#include "orb_pyramid.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

struct GatherDev { int key0, out0, n, kp0, level_index, frame; };   // a list: its candidates, its kept indices, where its keypoints go

__global__ __launch_bounds__(64) void k_extract_gather(const GatherDev* lists, const float2* cand_xy, const float* cand_response, const int* kept,
                                                       float2* xy, float* response, int* level_index, int* frame) {
  const GatherDev G = lists[blockIdx.x];
  for (int i = threadIdx.x; i < G.n; i += 64) {
    const int src = G.key0 + kept[G.out0 + i];
    const float2 p = cand_xy[src];
    xy[G.kp0 + i] = make_float2(p.x + (float)kFastBorder, p.y + (float)kFastBorder);
    response[G.kp0 + i] = cand_response[src];
    level_index[G.kp0 + i] = G.level_index; frame[G.kp0 + i] = G.frame;
  }
}

struct ExtractState {
  StagedCall call;   // [lists | levels | blur plan | tiles | tables] in, [xy | response | angle | descriptors] out, the rest as work
  double ms[4] = {0, 0, 0, 0};
  double ms_tail[5] = {0, 0, 0, 0, 0};   // of the last call with a tail: the four phases without the tail, then the tail
};

// What the call checks itself; the image, n_levels and inv_scale are osh_orb_pyramid_build's to refuse
static int extract_validate(int k, const osh_extract_frame& f, const osh_extract_result& r) {
  const char* entry = "osh_orb_extract";
  if (f.ini_th < 1 || f.ini_th > 255 || f.min_th < 1 || f.min_th > 255) { set_error("%s: frame %d: threshold outside [1, 255]", entry, k); return OSH_ERR_INVALID; }
  if (f.min_th > f.ini_th) { set_error("%s: frame %d: min_th %d > ini_th %d", entry, k, f.min_th, f.ini_th); return OSH_ERR_INVALID; }
  if (r.capacity < 0 || !r.level_count) { set_error("%s: frame %d: negative capacity or NULL level_count", entry, k); return OSH_ERR_INVALID; }
  if (r.capacity && (!r.xy || !r.level || !r.response || !r.angle || !r.size || !r.descriptors)) { set_error("%s: frame %d: NULL result array with capacity %d", entry, k, r.capacity); return OSH_ERR_INVALID; }
  if (!f.pattern) { set_error("%s: frame %d: NULL pattern", entry, k); return OSH_ERR_INVALID; }
  for (int i = 0; i < 2 * kBriefPoints; ++i)
    if (f.pattern[i] < -kBriefMaxCoord || f.pattern[i] > kBriefMaxCoord) { set_error("%s: frame %d: table point %d outside [-%d, %d]", entry, k, i / 2, kBriefMaxCoord, kBriefMaxCoord); return OSH_ERR_INVALID; }
  // a kept corner is at least minBorder + 3 = 19 pixels from every edge of its level: what the table may reach
  if (brief_reach(f.pattern) > kFastBorder + 3) { set_error("%s: frame %d: the table reaches %d pixels, more than %d", entry, k, brief_reach(f.pattern), kFastBorder + 3); return OSH_ERR_INVALID; }
  if (f.blur_q8) {
    int sum = 0;
    for (int u = 0; u < kBriefTaps; ++u) sum += f.blur_q8[u];
    if (sum != 256) { set_error("%s: frame %d: the blur weights sum to %d, not 256", entry, k, sum); return OSH_ERR_INVALID; }
  }
  if (f.n_levels < 1 || f.n_levels > OSH_STEREO_MAX_LEVELS) { set_error("%s: frame %d: n_levels %d outside [1, %d]", entry, k, f.n_levels, OSH_STEREO_MAX_LEVELS); return OSH_ERR_INVALID; }
  if (!f.scale || !f.n_features) { set_error("%s: frame %d: NULL scale or n_features", entry, k); return OSH_ERR_INVALID; }
  for (int l = 0; l < f.n_levels; ++l) {
    if (!std::isfinite(f.scale[l]) || !(f.scale[l] > 0.f) || f.scale[l] > 1.0e6f) { set_error("%s: frame %d: scale[%d] is not a finite positive number", entry, k, l); return OSH_ERR_INVALID; }
    if (f.n_features[l] > kOctMaxFeatures) { set_error("%s: frame %d: n_features[%d] above OSH_OCTREE_MAX_FEATURES", entry, k, l); return OSH_ERR_UNSUPPORTED; }
  }
  return OSH_OK;
}

// The body of osh_orb_extract and osh_orb_extract_raw (orb_prepare_device.hip): they differ in where level 0 comes from
int extract_from(const char* entry, osh_orb_ctx* c, int32_t n_frames, const osh_extract_frame* frames, osh_extract_result* results, const Level0Producer* producer,
                 const ExtractTail* tail) {
  PhaseClock clock;
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  for (int k = 0; k < n_frames; ++k) OSH_TRY(extract_validate(k, frames[k], results[k]));   // a refusal needs no context and no device
  if (tail && tail->order.size() != (size_t)n_frames) { set_error("%s: the tail orders %zu frames of %d", entry, tail->order.size(), n_frames); return OSH_ERR_INVALID; }
  // the pyramid: exactly an osh_orb_pyramid_build, which refuses what it refuses before it touches the resident pyramid
  std::vector<osh_pyramid_frame> pf((size_t)n_frames);
  std::vector<osh_pyramid_result> pr((size_t)n_frames);
  for (int k = 0; k < n_frames; ++k) {
    pf[k] = {frames[k].image, frames[k].n_levels, frames[k].inv_scale};
    pr[k] = {0, nullptr, nullptr, results[k].levels, results[k].border};
  }
  OSH_TRY(pyramid_build_from(c, n_frames, pf.data(), pr.data(), producer));
  if (n_frames == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  ExtractState* st = orb_state<ExtractState>(c, kOrbAttachExtract);
  clock.profiling = orb_profiling(c);
  clock.mark();

  // the detector on the resident levels
  std::vector<osh_fast_resident_frame> rf((size_t)n_frames);
  for (int k = 0; k < n_frames; ++k) rf[k] = {pr[k].pyramid_token, frames[k].ini_th, frames[k].min_th};
  FastEmitted e;
  OSH_TRY(fast_emit_resident(entry, c, s, n_frames, rf.data(), e));
  clock.mark();

  // the octree of every level that has candidates, in (frame, level) order
  std::vector<OctListDev> lists;
  std::vector<GatherDev> gather;
  for (int k = 0; k < n_frames; ++k)
    for (int l = e.level0[k]; l < e.level0[k + 1]; ++l) {
      const EmittedLevel& L = e.levels[l];
      if (L.n == 0) continue;
      const int W = L.cols - 2 * kFastBorder, H = L.rows - 2 * kFastBorder;   // maxBorderX - minBorderX: positive, the level has cells
      if (L.n > kOctMaxKeys || oct_n_ini(W, H) > kOctMaxRoots) { set_error("%s: frame %d level %d: %d candidates or an area %d x %d beyond the octree's limits", entry, k, l - e.level0[k], L.n, W, H); return OSH_ERR_UNSUPPORTED; }
      lists.push_back({L.key0, L.n, W, H, frames[k].n_features[l - e.level0[k]], 0, 0});
      gather.push_back({L.key0, 0, 0, 0, l, k});
    }
  std::vector<int> count, status;
  const int* d_kept = nullptr;
  if (!lists.empty()) OSH_TRY(octree_run(c, s, lists, e.xy, e.response, count, status, &d_kept));
  std::vector<int> level_count(e.levels.size(), 0);
  // frame k's keypoints are [frame_kp0[k], frame_kp0[k] + frame_n[k]): frame after frame, or in the order a tail asks for
  std::vector<size_t> frame_kp0((size_t)n_frames, 0), frame_n((size_t)n_frames, 0), frame_list0((size_t)n_frames + 1, 0);
  for (size_t at = 0, k = 0; k <= (size_t)n_frames; ++k) {
    frame_list0[k] = at;
    for (; k < (size_t)n_frames && at < gather.size() && gather[at].frame == (int)k; ++at) {
      if (status[at] != OSH_OK) { set_error("%s: frame %d: an octree list reached a loop bound", entry, (int)k); return status[at]; }
      frame_n[k] += (size_t)count[at];
    }
  }
  size_t K = 0;
  for (int j = 0; j < n_frames; ++j) {
    const int k = tail ? tail->order[j] : j;
    frame_kp0[k] = K;
    for (size_t at = frame_list0[k]; at < frame_list0[k + 1]; ++at) {
      gather[at].out0 = lists[at].out0; gather[at].n = count[at]; gather[at].kp0 = (int)K;
      level_count[gather[at].level_index] = count[at];
      K += (size_t)count[at];
    }
  }
  clock.mark();

  // orientation, blur and descriptors of the kept keypoints
  const size_t n_levels = e.levels.size();
  size_t blur_bytes = 0;
  std::vector<size_t> blur_off(n_levels);
  std::vector<BlurTileDev> tiles;
  for (size_t l = 0; l < n_levels; ++l) {
    blur_off[l] = blur_bytes;
    blur_bytes += (size_t)e.levels[l].rows * e.levels[l].cols;
    if (level_count[l]) blur_tiles((int)l, e.levels[l].rows, e.levels[l].cols, tiles);
  }
  Layout in, out, work;
  const auto s_gather = in.take<GatherDev>(gather.size());
  const auto s_levels = in.take<PyramidLevelDev>(n_levels);
  const auto s_blurred = in.take<PyramidLevelDev>(n_levels);
  const auto s_blur = in.take<BlurLevelDev>(n_levels);
  const auto s_tiles = in.take<BlurTileDev>(tiles.size());
  const auto s_pattern = in.take<signed char>((size_t)n_frames * 2 * kBriefPoints);
  const auto o_xy = out.take<float2>(K); const auto o_resp = out.take<float>(K); const auto o_angle = out.take<float>(K);
  const auto o_desc = out.take<unsigned long long>(K * 4);
  const auto w_index = work.take<int>(K); const auto w_frame = work.take<int>(K);
  const auto w_m10 = work.take<int>(K); const auto w_m01 = work.take<int>(K); const auto w_cs = work.take<float2>(K);
  double tail_ms = 0;
  if (K) {
    if (tail) OSH_TRY(tail->plan(e, frame_kp0, frame_n, in, out, work));   // after the call's own sections: those stay where they are
    OSH_TRY(st->call.reserve(in, out, work.bytes));
    unsigned char* blurred = brief_blurred(c, blur_bytes);
    if (!blurred) return OSH_ERR_DEVICE;
    char* h = st->call.host_in();
    std::memcpy(s_gather.in(h), gather.data(), sizeof(GatherDev) * gather.size());
    for (int k = 0; k < n_frames; ++k) {
      for (int l = e.level0[k]; l < e.level0[k + 1]; ++l) {
        const EmittedLevel& L = e.levels[l];
        s_levels.in(h)[l] = {e.images + L.img_off, L.rows, L.cols};
        s_blur.in(h)[l] = blur_level(e.images + L.img_off, blurred + blur_off[l], L.rows, L.cols, frames[k].blur_q8);
        s_blurred.in(h)[l] = {blurred + blur_off[l], L.rows, L.cols};
      }
      std::memcpy(s_pattern.in(h) + (size_t)k * 2 * kBriefPoints, frames[k].pattern, 2 * kBriefPoints);
    }
    if (!tiles.empty()) std::memcpy(s_tiles.in(h), tiles.data(), sizeof(BlurTileDev) * tiles.size());
    if (tail) tail->stage(h);
    OSH_TRY(st->call.upload(s));
    char* di = st->call.dev_in(); char* dout = st->call.dev_out(); char* dw = st->call.dev_work();
    hipLaunchKernelGGL(k_extract_gather, dim3((unsigned)gather.size()), dim3(64), 0, s, s_gather.in(di), e.xy, e.response, d_kept, o_xy.in(dout), o_resp.in(dout),
                       w_index.in(dw), w_frame.in(dw));
    OSH_TRY(launch_check("extract gather"));
    OSH_TRY(ic_angle_launch(s, (int)K, s_levels.in(di), w_index.in(dw), o_xy.in(dout), o_angle.in(dout), w_m10.in(dw), w_m01.in(dw)));
    BriefView v{};
    v.n = (int)K; v.levels = s_blurred.in(di); v.level_index = w_index.in(dw); v.frame = w_frame.in(dw); v.xy = o_xy.in(dout);
    v.angle = o_angle.in(dout); v.pattern = s_pattern.in(di); v.desc = o_desc.in(dout); v.cos_sin = w_cs.in(dw);
    OSH_TRY(brief_launch(s, tiles.size(), s_blur.in(di), s_tiles.in(di), v));
    if (tail) {
      if (clock.profiling) OSH_HIP(hipStreamSynchronize(s));
      const PhaseClock::clk::time_point t0 = PhaseClock::clk::now();
      OSH_TRY(tail->launch(s, di, dout, dw, ExtractKept{K, o_xy.in(dout), w_index.in(dw), o_desc.in(dout), e.images}));
      if (clock.profiling) OSH_HIP(hipStreamSynchronize(s));
      tail_ms = std::chrono::duration<double, std::milli>(PhaseClock::clk::now() - t0).count();
    }
    OSH_TRY(st->call.download(s));   // synchronises
  }
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_frames; ++k) {
    osh_extract_result& r = results[k];
    const osh_extract_frame& f = frames[k];
    const size_t base = frame_kp0[k], n = frame_n[k];
    r.n_out = (int32_t)n; r.pyramid_token = pr[k].pyramid_token;
    for (int l = 0; l < f.n_levels; ++l) r.level_count[l] = level_count[e.level0[k] + l];
    if (n > (size_t)r.capacity) continue;   // counts only: the caller sizes its arrays and calls again
    scatter(reinterpret_cast<float2*>(r.xy), o_xy, ho, base, n); scatter(r.response, o_resp, ho, base, n); scatter(r.angle, o_angle, ho, base, n);
    scatter(reinterpret_cast<unsigned long long*>(r.descriptors), o_desc, ho, base, n, 4);
    size_t i = 0;
    for (int l = 0; l < f.n_levels; ++l) {
      const float diameter = (float)(int)(31 * f.scale[l]);   // :888: the patch diameter at the level's scale, cut to int
      for (int j = 0; j < r.level_count[l]; ++j, ++i) { r.level[i] = l; r.size[i] = diameter; }
    }
  }
  if (tail && K) tail->collect(ho);
  clock.mark();
  clock.store(st->ms);
  if (tail && clock.profiling) {
    for (int k = 0; k < 4; ++k) st->ms_tail[k] = st->ms[k];
    st->ms_tail[3] -= tail_ms; st->ms_tail[4] = tail_ms;
  }
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_extract(osh_orb_ctx* c, int32_t n_frames, const osh_extract_frame* frames, osh_extract_result* results) {
  return extract_from("osh_orb_extract", c, n_frames, frames, results, nullptr);
}

extern "C" int osh_orb_extract_stereo_get_times(osh_orb_ctx* c, double ms[5]) {
  if (!c || !ms) { set_error("osh_orb_extract_stereo_get_times: bad arguments"); return OSH_ERR_INVALID; }
  std::memcpy(ms, orb_state<ExtractState>(c, kOrbAttachExtract)->ms_tail, sizeof(double) * 5);
  return OSH_OK;
}

extern "C" int osh_orb_extract_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<ExtractState>("osh_orb_extract_get_times", c, kOrbAttachExtract, ms);
}
