// fisheye_stereo_device.hip -- Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1131-1171) on MI355X (gfx950) for a batch of
// KannalaBrandt8 rig frames, and KannalaBrandt8::TriangulateMatches alone for explicit pairs.
//
// Two kernels per call, every frame of the batch in each:
//   k_fstereo_knn   the two nearest right keypoints >= mono_right of every left keypoint >= mono_left (BFmatcher.knnMatch(.., 2),
//                   :1149): one query per lane, the right descriptors staged through LDS, the right set cut into slices (grid z);
//                   every (slice, query) writes its own partial (nearest key, second distance), so nothing is merged by atomics and
//                   no buffer has to be preset.
//   k_fstereo_tri   one left keypoint per lane: the slices merged in ascending order (the lowest right index wins among equal
//                   distances), Lowe's test (:1156), kb8_triangulate_match (kb8_triangulate.h), depth > 0.0001f (:1162) and the
//                   scatter: every per-left output is written by its own lane, mvRightToLeftMatch by an integer atomicMax on an
//                   array the call preset to -1 (the reference's loop ascends in l and its last writer stays: the largest l).
// Lanes whose keypoint fails the ratio test idle through the triangulation of their wavefront's survivors.
#include "common.h"
#include "kb8_triangulate.h"
#include "orb_hamming.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

constexpr unsigned kFNone = 0xFFFFFFFFu;
constexpr int kFBlock = 64;    // left keypoints per block (one per lane of one wavefront)
constexpr int kFTile = 256;    // right keypoints staged in LDS per tile: 8 KiB of descriptors

struct FStereoFrameDev {
  int n_left, n_right, mono_left, mono_right, left_base, right_base;   // bases: offsets of this frame in the arrays of the batch
  int n_levels;
  float sigma2[OSH_STEREO_MAX_LEVELS];
  Kb8Rig rig;
};

struct FStereoView {
  int n_frames, n_split;
  size_t n_left_total;
  const FStereoFrameDev* frames;
  const float2* lxy; const int* loct; const uint4* ldesc;
  const float2* rxy; const int* roct; const uint4* rdesc;
  uint2* part;          // [n_split][n_left_total]: (distance << 22 | right index) of the slice's nearest, its second distance; kFNone: none
  int* l2r; int* r2l; float* depth; float* p3d;
  int* best_right; int* best_dist; int* second_dist; float* cosp; unsigned char* stage;
};

// grid = (ceil(max queries / 64), n_frames, n_split); block z searches one slice of the right keypoints >= mono_right
__global__ __launch_bounds__(kFBlock) void k_fstereo_knn(FStereoView v) {
  __shared__ uint4 sh_desc[kFTile * 2];
  const FStereoFrameDev& f = v.frames[blockIdx.y];
  const int n_query = f.n_left - f.mono_left, n_train = f.n_right - f.mono_right;
  if ((int)blockIdx.x * kFBlock >= n_query) return;   // block-uniform
  const int q = blockIdx.x * kFBlock + threadIdx.x;
  const bool valid = q < n_query;
  const size_t gl = (size_t)f.left_base + f.mono_left + (valid ? q : 0);
  const uint4 a0 = v.ldesc[gl * 2], a1 = v.ldesc[gl * 2 + 1];
  const int per = (n_train + (int)gridDim.z - 1) / (int)gridDim.z;
  const int t_begin = min(n_train, (int)blockIdx.z * per), t_end = min(n_train, t_begin + per);
  unsigned d1 = kFNone, i1 = 0, d2 = kFNone;
  for (int t0 = t_begin; t0 < t_end; t0 += kFTile) {
    const int nt = min(kFTile, t_end - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < nt * 2; k += kFBlock) sh_desc[k] = v.rdesc[((size_t)f.right_base + f.mono_right + t0) * 2 + k];
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const unsigned d = hamming256(a0, a1, sh_desc[2 * t], sh_desc[2 * t + 1]);   // wave-wide broadcast reads
      if (d < d1) { d2 = d1; d1 = d; i1 = (unsigned)(f.mono_right + t0 + t); }
      else if (d < d2) d2 = d;
    }
  }
  if (valid) v.part[(size_t)blockIdx.z * v.n_left_total + gl] = make_uint2(d1 == kFNone ? kFNone : (d1 << kPosBits) | i1, d2);
}

// grid = (ceil(max n_left / 64), n_frames)
__global__ __launch_bounds__(kFBlock) void k_fstereo_tri(FStereoView v) {
#pragma clang fp contract(off)
  const FStereoFrameDev& f = v.frames[blockIdx.y];
  const int l = blockIdx.x * kFBlock + threadIdx.x;
  if (l >= f.n_left) return;
  const size_t gl = (size_t)f.left_base + l;
  int stage, br = -1, bd = -1, sd = -1, match = -1;
  float cosp = OSH_FSTEREO_NO_COS, depth = -1.f, p3d[3] = {0.f, 0.f, 0.f};
  if (l < f.mono_left) {
    stage = OSH_FSTEREO_OUTSIDE;
  } else if (f.n_right - f.mono_right < 2) {
    stage = OSH_FSTEREO_NO_PAIR;                       // (*it).size() >= 2 (:1156)
  } else {
    unsigned d1 = kFNone, i1 = 0, d2 = kFNone;
    for (int z = 0; z < v.n_split; ++z) {              // ascending slices: a later equal distance never displaces an earlier one
      const uint2 p = v.part[(size_t)z * v.n_left_total + gl];
      if (p.x == kFNone) continue;
      const unsigned d = p.x >> kPosBits;
      if (d < d1) { d2 = d1; d1 = d; i1 = p.x & kPosMask; }
      else if (d < d2) d2 = d;
      if (p.y < d2) d2 = p.y;
    }
    br = (int)i1; bd = (int)d1; sd = (int)d2;
    if (!((double)(float)bd < (double)(float)sd * 0.7)) {   // (*it)[0].distance < (*it)[1].distance * 0.7 (:1156)
      stage = OSH_FSTEREO_RATIO;
    } else {
      const float2 pl = v.lxy[gl], pr = v.rxy[(size_t)f.right_base + br];
      const float sigma1 = f.sigma2[v.loct[gl]], sigma2 = f.sigma2[v.roct[(size_t)f.right_base + br]];   // :1160
      float x3D[3];
      const float ret = kb8_triangulate_match(f.rig, pl.x, pl.y, pr.x, pr.y, sigma1, sigma2, x3D, &cosp);
      if (ret == -1.f) stage = OSH_FSTEREO_PARALLAX;
      else if (ret == -2.f) stage = OSH_FSTEREO_BEHIND_1;
      else if (ret == -3.f) stage = OSH_FSTEREO_BEHIND_2;
      else if (ret == -4.f) stage = OSH_FSTEREO_REPROJ_1;
      else if (ret == -5.f) stage = OSH_FSTEREO_REPROJ_2;
      else if (!(ret > 0.0001f)) stage = OSH_FSTEREO_DEPTH;   // :1162
      else {
        stage = OSH_FSTEREO_ACCEPTED;
        match = br; depth = ret; p3d[0] = x3D[0]; p3d[1] = x3D[1]; p3d[2] = x3D[2];
        atomicMax(&v.r2l[(size_t)f.right_base + br], l);      // :1164, last writer of an ascending loop
      }
    }
  }
  v.l2r[gl] = match; v.depth[gl] = depth;
  v.p3d[gl * 3] = p3d[0]; v.p3d[gl * 3 + 1] = p3d[1]; v.p3d[gl * 3 + 2] = p3d[2];
  v.best_right[gl] = br; v.best_dist[gl] = bd; v.second_dist[gl] = sd; v.cosp[gl] = cosp;
  v.stage[gl] = (unsigned char)stage;
}

// TriangulateMatches for n explicit pairs of one rig, one pair per lane
__global__ __launch_bounds__(kFBlock) void k_kb8_triangulate(Kb8Rig rig, int n, const float2* xy1, const float2* xy2, const float* sigma1,
                                                            const float* sigma2, float* ret, float* p3d, float* cosp) {
  const int i = blockIdx.x * kFBlock + threadIdx.x;
  if (i >= n) return;
  float x3D[3], c;
  ret[i] = kb8_triangulate_match(rig, xy1[i].x, xy1[i].y, xy2[i].x, xy2[i].y, sigma1[i], sigma2[i], x3D, &c);
  p3d[3 * (size_t)i] = x3D[0]; p3d[3 * (size_t)i + 1] = x3D[1]; p3d[3 * (size_t)i + 2] = x3D[2];
  cosp[i] = c;
}

struct FStereoState {
  StagedCall call, tri;
  double ms[4] = {0, 0, 0, 0};
};

static bool all_finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
  return true;
}

static int rig_validate(const char* who, int k, const float* cam1, const float* cam2, float prec1, float prec2, const float* R, const float* t) {
  if (!all_finite(cam1, 8) || !all_finite(cam2, 8) || !std::isfinite(prec1) || !std::isfinite(prec2) || !all_finite(R, 9) || !all_finite(t, 3)) {
    set_error("%s %d: a camera parameter, precision or entry of the relative pose is not finite", who, k); return OSH_ERR_INVALID;
  }
  if (cam1[0] == 0.f || cam1[1] == 0.f || cam2[0] == 0.f || cam2[1] == 0.f) { set_error("%s %d: fx or fy is 0", who, k); return OSH_ERR_INVALID; }
  return OSH_OK;
}

static int fstereo_validate(int n_frames, const osh_fisheye_stereo_frame* frames, const osh_fisheye_stereo_result* results) {
  for (int k = 0; k < n_frames; ++k) {
    const osh_fisheye_stereo_frame& f = frames[k];
    const osh_fisheye_stereo_result& r = results[k];
    if (f.n_left < 0 || f.n_right < 0) { set_error("frame %d: negative keypoint count", k); return OSH_ERR_INVALID; }
    if (f.mono_left < 0 || f.mono_left > f.n_left) { set_error("frame %d: mono_left %d outside [0, %d]", k, f.mono_left, f.n_left); return OSH_ERR_INVALID; }
    if (f.mono_right < 0 || f.mono_right > f.n_right) { set_error("frame %d: mono_right %d outside [0, %d]", k, f.mono_right, f.n_right); return OSH_ERR_INVALID; }
    OSH_TRY(validate_keypoint_sides(k, f, kPosMask));
    if (!f.level_sigma2) { set_error("frame %d: NULL level_sigma2", k); return OSH_ERR_INVALID; }
    if (f.n_left && (!f.left_xy || !f.left_octave || !f.left_desc || !r.left_to_right || !r.depth || !r.p3d)) { set_error("frame %d: NULL left keypoint or result array", k); return OSH_ERR_INVALID; }
    if (f.n_right && (!f.right_xy || !f.right_octave || !f.right_desc || !r.right_to_left)) { set_error("frame %d: NULL right keypoint or result array", k); return OSH_ERR_INVALID; }
    if (!all_finite(f.level_sigma2, (size_t)f.n_levels)) { set_error("frame %d: level_sigma2 entry not finite", k); return OSH_ERR_INVALID; }
    OSH_TRY(rig_validate("frame", k, f.cam1, f.cam2, f.precision1, f.precision2, f.Rlr, f.tlr));
    if (!all_finite(f.left_xy, (size_t)f.n_left * 2) || !all_finite(f.right_xy, (size_t)f.n_right * 2)) { set_error("frame %d: keypoint coordinate not finite", k); return OSH_ERR_INVALID; }
    OSH_TRY(validate_octaves(k, "left", f.left_octave, f.n_left, f.n_levels));
    OSH_TRY(validate_octaves(k, "right", f.right_octave, f.n_right, f.n_levels));
  }
  return OSH_OK;
}

static void fill_rig(Kb8Rig& g, const float* cam1, const float* cam2, float prec1, float prec2, const float* R, const float* t) {
  std::memcpy(g.cam1, cam1, sizeof g.cam1); std::memcpy(g.cam2, cam2, sizeof g.cam2);
  g.prec1 = prec1; g.prec2 = prec2;
  std::memcpy(g.R12, R, sizeof g.R12); std::memcpy(g.t12, t, sizeof g.t12);
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_fisheye_stereo_match(osh_orb_ctx* c, int32_t n_frames, const osh_fisheye_stereo_frame* frames,
                                            const osh_fisheye_stereo_result* results) {
  PhaseClock clock;
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_fisheye_stereo_match: bad arguments"); return OSH_ERR_INVALID; }
  OSH_TRY(fstereo_validate(n_frames, frames, results));   // the frames first: a refusal needs no context and no device
  if (!c) { set_error("osh_orb_fisheye_stereo_match: no context"); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  FStereoState* st = orb_state<FStereoState>(c, kOrbAttachFisheye);
  clock.profiling = orb_profiling(c);

  KeypointBatch kb;
  OSH_TRY(kb.size("osh_orb_fisheye_stereo_match", n_frames, frames));
  const size_t NL = kb.NL, NR = kb.NR;
  int max_query = 0, max_train = 0;
  std::vector<FStereoFrameDev> fd(n_frames);
  for (int k = 0; k < n_frames; ++k) {
    const osh_fisheye_stereo_frame& f = frames[k];
    FStereoFrameDev& d = fd[k];
    std::memset(&d, 0, sizeof d);
    d.n_left = f.n_left; d.n_right = f.n_right; d.mono_left = f.mono_left; d.mono_right = f.mono_right;
    d.left_base = kb.base[k].left; d.right_base = kb.base[k].right; d.n_levels = f.n_levels;
    for (int l = 0; l < OSH_STEREO_MAX_LEVELS; ++l) d.sigma2[l] = l < f.n_levels ? f.level_sigma2[l] : 1.f;
    fill_rig(d.rig, f.cam1, f.cam2, f.precision1, f.precision2, f.Rlr, f.tlr);
    max_query = std::max(max_query, f.n_left - f.mono_left);
    max_train = std::max(max_train, f.n_right - f.mono_right);
  }
  // a single 1000 + 1000 frame becomes 16 x 4 = 64 one-wavefront blocks, which does not fill the 256 CUs (a frame is only 10^6 distances)
  const int qblocks = (max_query + kFBlock - 1) / kFBlock;
  const int split = right_set_slices(qblocks, n_frames, max_train, kFTile);

  Layout in, out, work;
  const auto s_frames = in.take<FStereoFrameDev>(n_frames);
  kb.take(in);
  const auto o_l2r = out.take<int>(NL); const auto o_r2l = out.take<int>(NR); const auto o_depth = out.take<float>(NL);
  const auto o_p3d = out.take<float>(NL * 3); const auto o_br = out.take<int>(NL); const auto o_bd = out.take<int>(NL);
  const auto o_sd = out.take<int>(NL); const auto o_cos = out.take<float>(NL); const auto o_stage = out.take<unsigned char>(NL);
  const auto w_part = work.take<uint2>(NL * (size_t)split);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  std::memcpy(s_frames.in(h), fd.data(), sizeof(FStereoFrameDev) * n_frames);
  kb.stage(h, frames);
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  char* dout = st->call.dev_out();
  if (NR) OSH_HIP(hipMemsetAsync(o_r2l.in(dout), 0xFF, NR * 4, s));   // -1: the floor of the atomicMax
  if (NL) {
    FStereoView v{};
    char* di = st->call.dev_in();
    v.n_frames = n_frames; v.n_split = split; v.n_left_total = NL;
    v.frames = s_frames.in(di);
    kb.bind(v, di);
    v.part = w_part.in(st->call.dev_work());
    v.l2r = o_l2r.in(dout); v.r2l = o_r2l.in(dout); v.depth = o_depth.in(dout); v.p3d = o_p3d.in(dout);
    v.best_right = o_br.in(dout); v.best_dist = o_bd.in(dout); v.second_dist = o_sd.in(dout); v.cosp = o_cos.in(dout); v.stage = o_stage.in(dout);
    if (qblocks > 0 && max_train >= 2)
      hipLaunchKernelGGL(k_fstereo_knn, dim3((unsigned)qblocks, (unsigned)n_frames, (unsigned)split), dim3(kFBlock), 0, s, v);
    hipLaunchKernelGGL(k_fstereo_tri, dim3((unsigned)((kb.max_left + kFBlock - 1) / kFBlock), (unsigned)n_frames), dim3(kFBlock), 0, s, v);
    OSH_TRY(launch_check("fisheye stereo match"));
  }
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_frames; ++k) {
    const osh_fisheye_stereo_result& r = results[k];
    const size_t n = (size_t)frames[k].n_left, b = (size_t)kb.base[k].left;
    scatter(r.right_to_left, o_r2l, ho, (size_t)kb.base[k].right, (size_t)frames[k].n_right);
    scatter(r.left_to_right, o_l2r, ho, b, n); scatter(r.depth, o_depth, ho, b, n); scatter(r.p3d, o_p3d, ho, b, n, 3);
    scatter(r.best_right, o_br, ho, b, n); scatter(r.best_dist, o_bd, ho, b, n); scatter(r.second_dist, o_sd, ho, b, n);
    scatter(r.cos_parallax, o_cos, ho, b, n); scatter(r.stage, o_stage, ho, b, n);
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_fisheye_stereo_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<FStereoState>("osh_orb_fisheye_stereo_get_times", c, kOrbAttachFisheye, ms);
}

extern "C" int osh_kb8_triangulate(osh_orb_ctx* c, int32_t n, const osh_kb8_rig* rig, const float* xy1, const float* xy2, const float* sigma1,
                                   const float* sigma2, float* ret, float* p3d, float* cos_parallax) {
  if (n < 0 || !rig) { set_error("osh_kb8_triangulate: bad arguments"); return OSH_ERR_INVALID; }
  if (n > 0 && (!xy1 || !xy2 || !sigma1 || !sigma2 || !ret)) { set_error("osh_kb8_triangulate: NULL array with n = %d", n); return OSH_ERR_INVALID; }
  if ((size_t)n > (size_t)INT_MAX / 16) { set_error("osh_kb8_triangulate: n too large"); return OSH_ERR_UNSUPPORTED; }
  OSH_TRY(rig_validate("rig", 0, rig->cam1, rig->cam2, rig->precision1, rig->precision2, rig->R12, rig->t12));
  if (!all_finite(xy1, (size_t)n * 2) || !all_finite(xy2, (size_t)n * 2) || !all_finite(sigma1, (size_t)n) || !all_finite(sigma2, (size_t)n)) {
    set_error("osh_kb8_triangulate: coordinate or sigma not finite"); return OSH_ERR_INVALID;
  }
  if (!c) { set_error("osh_kb8_triangulate: no context"); return OSH_ERR_INVALID; }
  if (n == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  FStereoState* st = orb_state<FStereoState>(c, kOrbAttachFisheye);
  const size_t N = (size_t)n;
  Layout in, out;
  const auto s_xy1 = in.take<float2>(N); const auto s_xy2 = in.take<float2>(N); const auto s_s1 = in.take<float>(N); const auto s_s2 = in.take<float>(N);
  const auto o_ret = out.take<float>(N); const auto o_p3d = out.take<float>(N * 3); const auto o_cos = out.take<float>(N);
  OSH_TRY(st->tri.reserve(in, out));
  char* h = st->tri.host_in();
  std::memcpy(s_xy1.in(h), xy1, N * 8); std::memcpy(s_xy2.in(h), xy2, N * 8);
  std::memcpy(s_s1.in(h), sigma1, N * 4); std::memcpy(s_s2.in(h), sigma2, N * 4);
  OSH_TRY(st->tri.upload(s));
  Kb8Rig g;
  fill_rig(g, rig->cam1, rig->cam2, rig->precision1, rig->precision2, rig->R12, rig->t12);
  char* di = st->tri.dev_in(); char* dout = st->tri.dev_out();
  hipLaunchKernelGGL(k_kb8_triangulate, dim3((unsigned)((n + kFBlock - 1) / kFBlock)), dim3(kFBlock), 0, s, g, n, s_xy1.in(di), s_xy2.in(di),
                     s_s1.in(di), s_s2.in(di), o_ret.in(dout), o_p3d.in(dout), o_cos.in(dout));
  OSH_TRY(launch_check("kb8 triangulate"));
  OSH_TRY(st->tri.download(s));
  char* ho = st->tri.host_out();
  std::memcpy(ret, o_ret.in(ho), N * 4);
  if (p3d) std::memcpy(p3d, o_p3d.in(ho), N * 12);
  if (cos_parallax) std::memcpy(cos_parallax, o_cos.in(ho), N * 4);
  return OSH_OK;
}
