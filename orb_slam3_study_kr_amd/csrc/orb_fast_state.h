// orb_fast_state.h -- what osh_orb_fast_detect keeps on its context (orb_fast_device.hip): the staging of its calls and the packed
// pyramid of its last call, which stays resident under a token per frame.  osh_orb_ic_angle (same file) and osh_orb_describe
// (orb_brief_device.hip) read that copy instead of uploading the pyramid again; both also share the pyramid checks below.
#pragma once
#include "common.h"
#include "orb_stage.h"
#include <vector>

namespace osh {

struct FastLevelHost { long long img_off; int rows, cols, cell0, n_cells; };
struct FastFrameHost { int level0, n_levels, cell0, n_cells; };   // level0 / cell0: first entry of the frame in the call's lists

struct FastState {
  StagedCall call;              // detect: [cells | order | images] in, [count | offset | used_min] out, mask as work
  DevBuf emitted;               // xy, response, level, cell of the call
  PinBuf h_emitted;
  StagedCall ic_call;           // ic_angle: keypoints (and the pyramid, when the caller hands one over)
  // the resident pyramid of the last detect
  uint64_t token0 = 0;          // token of its frame 0; 0: none
  std::vector<FastFrameHost> frames;
  std::vector<FastLevelHost> levels;
  size_t img_off = 0;           // of the image section in call's in region
  double ms[4] = {0, 0, 0, 0}, ms_ic[4] = {0, 0, 0, 0};
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

// The frame of the resident pyramid that `token` names; nullptr: it names none of the context's last osh_orb_fast_detect
inline const FastFrameHost* fast_resident_frame(const FastState* st, uint64_t token) {
  if (!st->token0 || token < st->token0 || token - st->token0 >= (uint64_t)st->frames.size()) return nullptr;
  return &st->frames[(size_t)(token - st->token0)];
}
// First byte of the resident pyramid on the device; a level's pixels start FastLevelHost::img_off bytes further
inline const unsigned char* fast_resident_images(const FastState* st) {
  return reinterpret_cast<const unsigned char*>(st->call.dev_in()) + st->img_off;
}

}  // namespace osh
