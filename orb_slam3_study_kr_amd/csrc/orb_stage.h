// orb_stage.h -- the host code osh_orb_stereo_match (stereo_device.hip) and osh_orb_fisheye_stereo_match (fisheye_stereo_device.hip)
// share: both take a batch of frames with left and right ORB keypoints (xy, octave, 32-byte descriptor per keypoint), lay the frames'
// keypoints one after another in six arrays, run on an osh_orb_ctx attachment and time the same four host-clock phases.  Kernels,
// views, device frame descriptors, outputs and whatever a validator checks beyond the checks below stay with their entry.
// osh_orb_stereo_match_resident and the stereo tail of osh_orb_extract_stereo (stereo_device.hip) are the rectified matcher on
// resident pyramids: stereo_frame.h holds what the three rectified entries share beyond this file.
// osh_kb8_triangulate is not a client: it stages four flat arrays and no frames through a StagedCall of its own.
// osh_orb_bow_transform (bow_device.hip) has frames of descriptors only: it uses scatter, PhaseClock, orb_state and copy_times.
// osh_orb_bow_db_query (bowdb_device.hip) has queries against a database: it uses PhaseClock, orb_state and copy_times.
// osh_orb_triangulate_new_points (newpoint_device.hip) has segments of matched pairs: it uses scatter, PhaseClock, orb_state and copy_times.
// osh_orb_fast_detect / osh_orb_ic_angle (orb_fast_device.hip) and osh_orb_describe (orb_brief_device.hip) have pyramids, brought
// along or resident on the context: orb_pyramid_set.h, built on pack_level, is their level list; they use scatter, PhaseClock,
// orb_state and copy_times.  osh_orb_pyramid_build (orb_pyramid_device.hip) fills the resident pyramid: pack_level, PhaseClock, orb_state.
// osh_orb_prepare / osh_orb_extract_raw (orb_prepare_device.hip) have raw images and resident rectify maps: PhaseClock, orb_state, copy_times.
// osh_orb_refresh_map_points (mappoint_device.hip) has batches of map points: it uses scatter, PhaseClock, orb_state and copy_times.
// osh_orb_two_view_reconstruct (two_view_device.hip), osh_orb_mlpnp_solve (mlpnp_device.hip) and osh_orb_sim3_ransac
// (sim3_ransac_device.hip) have problems of correspondences and minimal sets: ransac_stage.h is their validator, batch bookkeeping and
// ballot loops; they use scatter, PhaseClock, orb_state and copy_times (MLPnP with five times).
// osh_orb_keyframe_cull_stage / _count (keyframe_cull_device.hip) keep one problem resident and count it under removed sets: they use
// PhaseClock, orb_state and copy_times.
#pragma once
#include "common.h"
#include <chrono>
#include <climits>
#include <vector>

namespace osh {

// The keypoints of a batch.  Frame: osh_stereo_frame or osh_fisheye_stereo_frame (n_left, n_right and the six arrays under the same names).
struct KeypointBatch {
  struct Base { int left, right; };   // offsets of one frame in the left and right arrays of the batch
  std::vector<Base> base;
  size_t NL = 0, NR = 0;
  int max_left = 0, max_right = 0;
  Section<float2> lxy, rxy;
  Section<int> loct, roct;
  Section<uint4> ldesc, rdesc;   // two per keypoint

  template <class Frame>
  int size(const char* entry, int n_frames, const Frame* frames) {
    base.resize(n_frames);
    for (int k = 0; k < n_frames; ++k) {
      base[k] = {(int)NL, (int)NR};
      NL += (size_t)frames[k].n_left; NR += (size_t)frames[k].n_right;
      max_left = std::max(max_left, frames[k].n_left); max_right = std::max(max_right, frames[k].n_right);
      if (NL > (size_t)INT_MAX / 16 || NR > (size_t)INT_MAX / 16) { set_error("%s: batch too large", entry); return OSH_ERR_UNSUPPORTED; }
    }
    return OSH_OK;
  }
  void take(Layout& in) {
    lxy = in.take<float2>(NL); loct = in.take<int>(NL); ldesc = in.take<uint4>(NL * 2);
    rxy = in.take<float2>(NR); roct = in.take<int>(NR); rdesc = in.take<uint4>(NR * 2);
  }
  template <class Frame>
  void stage(char* h, const Frame* frames) const {   // h: the host staging buffer; an empty side may hand over NULL arrays
    for (size_t k = 0; k < base.size(); ++k) {
      const Frame& f = frames[k];
      const size_t nl = (size_t)f.n_left, nr = (size_t)f.n_right, bl = (size_t)base[k].left, br = (size_t)base[k].right;
      if (nl) { std::memcpy(lxy.in(h) + bl, f.left_xy, nl * 8); std::memcpy(loct.in(h) + bl, f.left_octave, nl * 4); std::memcpy(ldesc.in(h) + bl * 2, f.left_desc, nl * 32); }
      if (nr) { std::memcpy(rxy.in(h) + br, f.right_xy, nr * 8); std::memcpy(roct.in(h) + br, f.right_octave, nr * 4); std::memcpy(rdesc.in(h) + br * 2, f.right_desc, nr * 32); }
    }
  }
  template <class View>
  void bind(View& v, char* dev_in) const {
    v.lxy = lxy.in(dev_in); v.loct = loct.in(dev_in); v.ldesc = ldesc.in(dev_in);
    v.rxy = rxy.in(dev_in); v.roct = roct.in(dev_in); v.rdesc = rdesc.in(dev_in);
  }
};

// The rows of a pyramid level (rows `stride` bytes apart) one after another at dst, stride = cols
inline void pack_level(unsigned char* dst, const osh_stereo_image& im) {
  if (im.stride == im.cols) { std::memcpy(dst, im.data, (size_t)im.rows * im.cols); return; }
  for (int r = 0; r < im.rows; ++r) std::memcpy(dst + (size_t)r * im.cols, im.data + (size_t)r * im.stride, (size_t)im.cols);
}

// `n` results of `per_item` values each from `section` of the downloaded outputs, for a frame whose results start at `base`
template <class T>
void scatter(T* dst, Section<T> section, const char* host_out, size_t base, size_t n, size_t per_item = 1) {
  if (dst && n) std::memcpy(dst, section.in(host_out) + base * per_item, n * per_item * sizeof(T));
}

// Slices of the right set (grid z of the search kernel): enough one-wavefront blocks to fill the device when the batch is a single
// frame (a 1000 + 1000 frame is 16 query blocks; 1024 blocks are aimed at), at most 16 slices, and no slice shorter than one LDS
// tile; a batch needs no slicing.  The max(1, ..) on the blocks serves a batch without a query; the rectified entry only asks with
// a left keypoint (NL > 0, so query_blocks >= 1), where it is a no-op.
inline int right_set_slices(int query_blocks, int n_frames, int max_train, int tile) {
  const long blocks = std::max<long>(1, (long)query_blocks * n_frames);
  const int split = (int)std::min<long>(16, std::max<long>(1, (1024 + blocks - 1) / blocks));
  return std::min(split, std::max(1, (max_train + tile - 1) / tile));
}

// The checks both validators make next to each other: the level count, and n_right against the position bits of a packed key.
template <class Frame>
int validate_keypoint_sides(int k, const Frame& f, unsigned pos_mask) {
  if (f.n_levels < 1 || f.n_levels > OSH_STEREO_MAX_LEVELS) { set_error("frame %d: n_levels %d outside [1, %d]", k, f.n_levels, OSH_STEREO_MAX_LEVELS); return OSH_ERR_INVALID; }
  if ((unsigned)f.n_right > pos_mask) { set_error("frame %d: n_right exceeds %u", k, pos_mask); return OSH_ERR_UNSUPPORTED; }
  return OSH_OK;
}
inline int validate_octaves(int k, const char* side, const int32_t* octave, int n, int n_levels) {
  for (int i = 0; i < n; ++i)
    if (octave[i] < 0 || octave[i] >= n_levels) { set_error("frame %d: %s octave %d outside [0, %d)", k, side, octave[i], n_levels); return OSH_ERR_INVALID; }
  return OSH_OK;
}

// The four host-clock phases of a call (staging, upload, kernels, download): constructed at the start, a mark at the end of each.
// Under profiling the marks that end a device phase synchronise the stream first, and store() keeps the times.
struct PhaseClock {
  using clk = std::chrono::steady_clock;
  bool profiling = false;
  clk::time_point t[5] = {clk::now()};
  int n = 1;
  void mark() { t[n++] = clk::now(); }
  int mark_synced(hipStream_t s) { if (profiling) OSH_HIP(hipStreamSynchronize(s)); mark(); return OSH_OK; }
  void store(double ms[4]) const { if (profiling) for (int k = 0; k < 4; ++k) ms[k] = std::chrono::duration<double, std::milli>(t[k + 1] - t[k]).count(); }
};

// The T an entry keeps in `slot` of the context: created on first use, deleted by osh_orb_destroy.
template <class T>
T* orb_state(osh_orb_ctx* c, OrbAttachSlot slot) {
  void** p = orb_attachment(c, [](void* q) { delete static_cast<T*>(q); }, slot);
  if (!*p) *p = new T();
  return static_cast<T*>(*p);
}
// osh_orb_*_get_times: the N times the last profiled call of the entry stored in its state's ms (the four phases first); zeros before any
template <class T, int N = 4>
int copy_times(const char* entry, osh_orb_ctx* c, OrbAttachSlot slot, double* ms) {
  if (!c || !ms) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  static_assert(sizeof(T::ms) == sizeof(double) * N, "the state keeps N times");
  std::memcpy(ms, orb_state<T>(c, slot)->ms, sizeof(double) * N);
  return OSH_OK;
}

}  // namespace osh
