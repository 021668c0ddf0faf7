// orb_fast_state.h -- what osh_orb_fast_detect keeps on its context (orb_fast_device.hip): the staging of its calls and the packed
// pyramid that stays resident under a token per frame.  The resident pyramid has a buffer of its own, filled either by the upload
// of an osh_orb_fast_detect or by the kernels of an osh_orb_pyramid_build (orb_pyramid_device.hip); each of the two replaces what
// the other left and takes its tokens from the same counter.  osh_orb_ic_angle and osh_orb_fast_detect_resident (orb_fast_device.hip)
// and osh_orb_describe (orb_brief_device.hip) read that copy instead of uploading the pyramid again; all share the pyramid checks
// below.
#pragma once
#include "common.h"
#include "orb_stage.h"
#include <atomic>
#include <vector>

namespace osh {

struct FastLevelHost { long long img_off; int rows, cols, cell0, n_cells; };
struct FastFrameHost { int level0, n_levels, cell0, n_cells; };   // level0 / cell0: first entry of the frame in the call's lists

inline std::atomic<uint64_t> g_fast_next_token{1};   // of every context: a token names one frame of one resident pyramid

struct FastState {
  StagedCall call;              // detect: [cells | order] in, [count | offset | used_min] out, mask as work
  DevBuf emitted;               // xy, response, level, cell of the call
  PinBuf h_emitted;
  StagedCall ic_call;           // ic_angle: keypoints (and the pyramid, when the caller hands one over)
  // the resident pyramid of the last detect or build: levels[].img_off are offsets into `resident`
  DevBuf resident;
  PinBuf h_images;              // detect: the packed levels on their way up; build: the packed images (level 0 of every frame)
  uint64_t token0 = 0;          // token of its frame 0; 0: none
  std::vector<FastFrameHost> frames;
  std::vector<FastLevelHost> levels;
  // osh_orb_pyramid_build
  StagedCall pyr_call;          // [jobs | taps | border jobs] in
  DevBuf bordered;              // the bordered levels of a build with a download
  PinBuf h_bordered;
  double ms[4] = {0, 0, 0, 0}, ms_ic[4] = {0, 0, 0, 0}, ms_pyr[4] = {0, 0, 0, 0};
};

inline int fast_validate_pyramid(const char* entry, int k, int n_levels, const osh_stereo_image* pyr) {
  if (n_levels < 1 || n_levels > OSH_STEREO_MAX_LEVELS) { set_error("%s: frame %d: n_levels %d outside [1, %d]", entry, k, n_levels, OSH_STEREO_MAX_LEVELS); return OSH_ERR_INVALID; }
  if (!pyr) { set_error("%s: frame %d: NULL pyramid", entry, k); return OSH_ERR_INVALID; }
  for (int l = 0; l < n_levels; ++l) {
    const osh_stereo_image& im = pyr[l];
    if (!im.data || im.rows <= 0 || im.cols <= 0 || im.stride < im.cols) { set_error("%s: frame %d: level %d is NULL, empty or has stride < cols", entry, k, l); return OSH_ERR_INVALID; }
    if (im.rows > OSH_FAST_MAX_SIDE || im.cols > OSH_FAST_MAX_SIDE) { set_error("%s: frame %d: level %d exceeds %d pixels in one direction", entry, k, l, OSH_FAST_MAX_SIDE); return OSH_ERR_UNSUPPORTED; }
  }
  return OSH_OK;
}

// The frame of the resident pyramid that `token` names; nullptr: it names none of the context's resident pyramid
inline const FastFrameHost* fast_resident_frame(const FastState* st, uint64_t token) {
  if (!st->token0 || token < st->token0 || token - st->token0 >= (uint64_t)st->frames.size()) return nullptr;
  return &st->frames[(size_t)(token - st->token0)];
}
// First byte of the resident pyramid on the device; a level's pixels start FastLevelHost::img_off bytes further
inline const unsigned char* fast_resident_images(const FastState* st) {
  return st->resident.as<const unsigned char>();
}

}  // namespace osh
