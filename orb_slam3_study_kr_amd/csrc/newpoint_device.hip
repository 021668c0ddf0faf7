// newpoint_device.hip -- the per-match body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:503-720) on MI355X (gfx950) for
// a batch of segments, a segment being one (current keyframe, neighbour) pair with its SearchForTriangulation matches.
//
// One kernel per call: k_newpoint_triangulate runs newpoint_triangulate (newpoint_triangulate.h) for one match per lane, blockIdx.y
// naming the segment.  The segment record (both keyframes' poses, cameras and level tables) is the same for a whole block and is read
// through scalar loads; the matches are arrays of the batch, one segment after another.  Every lane writes its own four outputs, so
// nothing has to be preset.  The Jacobi matrices of the null vector stay in registers as in k_fstereo_tri: no scratch.
#include "common.h"
#include "newpoint_triangulate.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

constexpr int kNpBlock = 64;   // matches per block (one per lane of one wavefront)

struct NpView {
  const NpSegment* seg;
  const int* idx1; const int* idx2;
  const float2* pt1; const float2* pt2;
  const int* oct1; const int* oct2;
  const float* ur1; const float* ur2; const float* d1; const float* d2;
  unsigned char* stage; unsigned char* source; float* cosp; float* x3d;
};

// grid = (ceil(max matches / 64), n_segments)
__global__ __launch_bounds__(kNpBlock) void k_newpoint_triangulate(NpView v) {
  const NpSegment& s = v.seg[blockIdx.y];
  const int i = blockIdx.x * kNpBlock + threadIdx.x;
  if (i >= s.n_matches) return;
  const size_t g = (size_t)s.base + i;
  const float2 p1 = v.pt1[g], p2 = v.pt2[g];
  const NpMatch m{v.idx1[g], v.idx2[g], p1.x, p1.y, p2.x, p2.y, v.oct1[g], v.oct2[g], v.ur1[g], v.ur2[g], v.d1[g], v.d2[g]};
  NpOut o;
  newpoint_triangulate(s, m, o);
  v.stage[g] = (unsigned char)o.stage; v.source[g] = (unsigned char)o.source; v.cosp[g] = o.cosp;
  v.x3d[g * 3] = o.x3D[0]; v.x3d[g * 3 + 1] = o.x3D[1]; v.x3d[g * 3 + 2] = o.x3D[2];
}

struct NewPointState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
};

static bool np_all_finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
  return true;
}

static int np_validate_camera(int k, const char* kf, const char* which, const osh_newpoint_camera& c) {
  if (c.type != OSH_NEWPOINT_PINHOLE && c.type != OSH_NEWPOINT_KB8) { set_error("segment %d: %s %s type %d is neither pinhole nor KannalaBrandt8", k, kf, which, c.type); return OSH_ERR_INVALID; }
  const bool kb8 = c.type == OSH_NEWPOINT_KB8;
  if (!np_all_finite(c.params, kb8 ? 8 : 4) || (kb8 && !std::isfinite(c.precision))) { set_error("segment %d: %s %s parameter not finite", k, kf, which); return OSH_ERR_INVALID; }
  if (c.params[0] == 0.f || c.params[1] == 0.f) { set_error("segment %d: %s %s fx or fy is 0", k, kf, which); return OSH_ERR_INVALID; }
  return OSH_OK;
}

static int np_validate_keyframe(int k, const char* kf, const osh_newpoint_keyframe& f) {
  const osh_newpoint_pose* poses[2] = {&f.pose, &f.right_pose};
  for (int p = 0; p < (f.has_camera2 ? 2 : 1); ++p)
    if (!np_all_finite(poses[p]->Rcw, 9) || !np_all_finite(poses[p]->tcw, 3) || !np_all_finite(poses[p]->Rwc, 9) || !np_all_finite(poses[p]->Ow, 3)) {
      set_error("segment %d: %s %spose entry not finite", k, kf, p ? "right " : ""); return OSH_ERR_INVALID;
    }
  OSH_TRY(np_validate_camera(k, kf, "camera", f.camera));
  if (f.has_camera2) OSH_TRY(np_validate_camera(k, kf, "camera2", f.camera2));
  const float scalars[8] = {f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy, f.mbf, f.mb};
  if (!np_all_finite(scalars, 8)) { set_error("segment %d: %s fx fy cx cy invfx invfy mbf mb: one is not finite", k, kf); return OSH_ERR_INVALID; }
  if (f.fx == 0.f || f.fy == 0.f) { set_error("segment %d: %s fx or fy is 0", k, kf); return OSH_ERR_INVALID; }
  if (f.n_keys < 0) { set_error("segment %d: %s negative n_keys", k, kf); return OSH_ERR_INVALID; }
  if (f.n_levels < 1 || f.n_levels > OSH_NEWPOINT_MAX_LEVELS) { set_error("segment %d: %s n_levels %d outside [1, %d]", k, kf, f.n_levels, OSH_NEWPOINT_MAX_LEVELS); return OSH_ERR_INVALID; }
  if (!f.level_sigma2 || !f.scale_factors) { set_error("segment %d: %s NULL level table", k, kf); return OSH_ERR_INVALID; }
  if (!np_all_finite(f.level_sigma2, (size_t)f.n_levels) || !np_all_finite(f.scale_factors, (size_t)f.n_levels)) { set_error("segment %d: %s level table entry not finite", k, kf); return OSH_ERR_INVALID; }
  return OSH_OK;
}

static int np_validate_side(int k, const char* kf, const osh_newpoint_keyframe& f, int n, const int32_t* idx, const int32_t* octave) {
  for (int i = 0; i < n; ++i) {
    if (idx[i] < 0 || idx[i] >= f.n_keys) { set_error("segment %d: match %d: index %d outside [0, %d) of %s", k, i, idx[i], f.n_keys, kf); return OSH_ERR_INVALID; }
    if (octave[i] < 0 || octave[i] >= f.n_levels) { set_error("segment %d: match %d: octave %d outside [0, %d) of %s", k, i, octave[i], f.n_levels, kf); return OSH_ERR_INVALID; }
  }
  return OSH_OK;
}

static int np_validate(int n_segments, const osh_newpoint_segment* segs, size_t* total, int* max_matches) {
  if (n_segments > OSH_NEWPOINT_MAX_SEGMENTS) { set_error("osh_orb_triangulate_new_points: more than %d segments", OSH_NEWPOINT_MAX_SEGMENTS); return OSH_ERR_UNSUPPORTED; }
  size_t N = 0;
  int mx = 0;
  for (int k = 0; k < n_segments; ++k) {
    const osh_newpoint_segment& s = segs[k];
    if (s.n_matches < 0) { set_error("segment %d: negative match count", k); return OSH_ERR_INVALID; }
    N += (size_t)s.n_matches; mx = std::max(mx, s.n_matches);
    if (N > (size_t)OSH_NEWPOINT_MAX_MATCHES) { set_error("osh_orb_triangulate_new_points: more than %d matches in one call", OSH_NEWPOINT_MAX_MATCHES); return OSH_ERR_UNSUPPORTED; }
    OSH_TRY(np_validate_keyframe(k, "kf1", s.kf1));
    OSH_TRY(np_validate_keyframe(k, "kf2", s.kf2));
    if (!std::isfinite(s.ratio_factor) || !std::isfinite(s.th_far_points)) { set_error("segment %d: ratio_factor or th_far_points not finite", k); return OSH_ERR_INVALID; }
    const size_t n = (size_t)s.n_matches;
    if (n && (!s.idx1 || !s.idx2 || !s.pt1 || !s.pt2 || !s.octave1 || !s.octave2 || !s.u_right1 || !s.u_right2 || !s.depth1 || !s.depth2)) {
      set_error("segment %d: NULL match array with n_matches = %d", k, s.n_matches); return OSH_ERR_INVALID;
    }
    if (!np_all_finite(s.pt1, n * 2) || !np_all_finite(s.pt2, n * 2)) { set_error("segment %d: keypoint coordinate not finite", k); return OSH_ERR_INVALID; }
    if (!np_all_finite(s.u_right1, n) || !np_all_finite(s.u_right2, n) || !np_all_finite(s.depth1, n) || !np_all_finite(s.depth2, n)) {
      set_error("segment %d: mvuRight or mvDepth entry not finite", k); return OSH_ERR_INVALID;
    }
    OSH_TRY(np_validate_side(k, "kf1", s.kf1, s.n_matches, s.idx1, s.octave1));
    OSH_TRY(np_validate_side(k, "kf2", s.kf2, s.n_matches, s.idx2, s.octave2));
  }
  *total = N; *max_matches = mx;
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_triangulate_new_points(osh_orb_ctx* c, int32_t n_segments, const osh_newpoint_segment* segs, const osh_newpoint_result* results) {
  PhaseClock clock;
  if (n_segments < 0 || (n_segments && (!segs || !results))) { set_error("osh_orb_triangulate_new_points: bad arguments"); return OSH_ERR_INVALID; }
  size_t N = 0;
  int max_matches = 0;
  OSH_TRY(np_validate(n_segments, segs, &N, &max_matches));   // the segments first: a refusal needs no context and no device
  if (!c) { set_error("osh_orb_triangulate_new_points: no context"); return OSH_ERR_INVALID; }
  if (N == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  NewPointState* st = orb_state<NewPointState>(c, kOrbAttachNewPoint);
  clock.profiling = orb_profiling(c);

  Layout in, out;
  const auto s_seg = in.take<NpSegment>((size_t)n_segments);
  const auto s_idx1 = in.take<int>(N); const auto s_idx2 = in.take<int>(N);
  const auto s_pt1 = in.take<float2>(N); const auto s_pt2 = in.take<float2>(N);
  const auto s_oct1 = in.take<int>(N); const auto s_oct2 = in.take<int>(N);
  const auto s_ur1 = in.take<float>(N); const auto s_ur2 = in.take<float>(N);
  const auto s_d1 = in.take<float>(N); const auto s_d2 = in.take<float>(N);
  const auto o_stage = out.take<unsigned char>(N); const auto o_source = out.take<unsigned char>(N);
  const auto o_cos = out.take<float>(N); const auto o_x3d = out.take<float>(N * 3);
  OSH_TRY(st->call.reserve(in, out));

  char* h = st->call.host_in();
  std::vector<size_t> base((size_t)n_segments);
  size_t b = 0;
  for (int k = 0; k < n_segments; ++k) {
    const osh_newpoint_segment& g = segs[k];
    const size_t n = (size_t)g.n_matches;
    base[k] = b;
    np_fill_segment(s_seg.in(h)[k], g, (int)b);
    if (n) {
      std::memcpy(s_idx1.in(h) + b, g.idx1, n * 4); std::memcpy(s_idx2.in(h) + b, g.idx2, n * 4);
      std::memcpy(s_pt1.in(h) + b, g.pt1, n * 8); std::memcpy(s_pt2.in(h) + b, g.pt2, n * 8);
      std::memcpy(s_oct1.in(h) + b, g.octave1, n * 4); std::memcpy(s_oct2.in(h) + b, g.octave2, n * 4);
      std::memcpy(s_ur1.in(h) + b, g.u_right1, n * 4); std::memcpy(s_ur2.in(h) + b, g.u_right2, n * 4);
      std::memcpy(s_d1.in(h) + b, g.depth1, n * 4); std::memcpy(s_d2.in(h) + b, g.depth2, n * 4);
    }
    b += n;
  }
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  NpView v{};
  v.seg = s_seg.in(di);
  v.idx1 = s_idx1.in(di); v.idx2 = s_idx2.in(di); v.pt1 = s_pt1.in(di); v.pt2 = s_pt2.in(di);
  v.oct1 = s_oct1.in(di); v.oct2 = s_oct2.in(di); v.ur1 = s_ur1.in(di); v.ur2 = s_ur2.in(di); v.d1 = s_d1.in(di); v.d2 = s_d2.in(di);
  v.stage = o_stage.in(dout); v.source = o_source.in(dout); v.cosp = o_cos.in(dout); v.x3d = o_x3d.in(dout);
  hipLaunchKernelGGL(k_newpoint_triangulate, dim3((unsigned)((max_matches + kNpBlock - 1) / kNpBlock), (unsigned)n_segments), dim3(kNpBlock), 0, s, v);
  OSH_TRY(launch_check("new point triangulation"));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_segments; ++k) {
    const osh_newpoint_result& r = results[k];
    const size_t n = (size_t)segs[k].n_matches;
    scatter(r.stage, o_stage, ho, base[k], n); scatter(r.source, o_source, ho, base[k], n);
    scatter(r.cos_parallax, o_cos, ho, base[k], n); scatter(r.x3d, o_x3d, ho, base[k], n, 3);
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_newpoint_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<NewPointState>("osh_orb_newpoint_get_times", c, kOrbAttachNewPoint, ms);
}
