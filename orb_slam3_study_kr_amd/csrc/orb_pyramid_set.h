// orb_pyramid_set.h -- where the pyramid levels of a call's frames are, for every entry that reads pyramids: in the context's
// resident pyramid under a token per frame, or brought along by the caller and uploaded with the call.  The resident pyramid is
// filled either by the upload of an osh_orb_fast_detect (orb_fast_device.hip) or by the kernels of an osh_orb_pyramid_build
// (orb_pyramid_device.hip); each replaces what the other left, through invalidate() and commit() below.  osh_orb_ic_angle and
// osh_orb_fast_detect_resident (orb_fast_device.hip) and osh_orb_describe (orb_brief_device.hip) read it by token.
// Host code only: no kernel and, apart from the DevBuf / PinBuf / StagedCall members of ResidentPyramid and FastState, no HIP call
// (`make pyramid-set-check` runs the rest in a plain host program).
#pragma once
#include "common.h"
#include "orb_fast.h"
#include "orb_stage.h"
#include <atomic>
#include <cmath>
#include <vector>

namespace osh {

struct FastLevelHost { long long img_off; int rows, cols, cell0, n_cells; };
struct FastFrameHost { int level0, n_levels, cell0, n_cells; };   // level0 / cell0: first entry of the frame in the call's lists

inline std::atomic<uint64_t> g_next_pyramid_token{1};   // of every context: a token names one frame of one resident pyramid

// The frames and levels of a resident pyramid (levels[].img_off are offsets from its first byte) and the protocol that replaces it
struct PyramidTable {
  uint64_t token0 = 0;          // token of its frame 0; 0: none
  std::vector<FastFrameHost> frames;
  std::vector<FastLevelHost> levels;
  // The frame that `token` names; nullptr: it names none of this pyramid
  const FastFrameHost* frame(uint64_t token) const {
    if (!token0 || token < token0 || token - token0 >= (uint64_t)frames.size()) return nullptr;
    return &frames[(size_t)(token - token0)];
  }
  // Before anything of the pyramid is overwritten: a call that fails from here on leaves none
  void invalidate() { token0 = 0; }
  // The new pyramid is complete: frame k has the token (return value) + k
  uint64_t commit(std::vector<FastFrameHost>&& f, std::vector<FastLevelHost>&& l) {
    frames = std::move(f); levels = std::move(l);
    return token0 = g_next_pyramid_token.fetch_add((uint64_t)frames.size());
  }
};
struct ResidentPyramid : PyramidTable {
  DevBuf buffer;
  PinBuf h_images;              // detect: the packed levels on their way up; build: the packed images (level 0 of every frame)
  const unsigned char* images() const { return buffer.as<const unsigned char>(); }   // its first byte on the device
};

struct FastState {
  StagedCall call;              // detect: [cells | order] in, [count | offset | used_min] out, mask as work
  DevBuf emitted;               // xy, response, level, cell of the call
  PinBuf h_emitted;
  StagedCall ic_call;           // ic_angle: keypoints (and the pyramid, when the caller hands one over)
  ResidentPyramid pyramid;      // of the last detect or build
  StagedCall pyr_call;          // osh_orb_pyramid_build: [jobs | taps | border jobs] in
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

struct PyramidLevelDev { const unsigned char* data; int rows, cols; };   // data: first pixel of the packed level on the device
// One level of a call; off: its first pixel, from the first byte of the resident pyramid or of the call's brought levels
struct PyramidLevel { bool resident; size_t off; int rows, cols; };

// Keypoints of frame k against its levels: finite, on a level of the frame, and the patch of reach R around the rounded centre
// inside that level.  `patch`: what the message calls it ("disc", "square")
inline int validate_keypoints(const char* entry, int k, int n, const float* xy, const int32_t* level, int n_levels, const PyramidLevel* lv, int R, const char* patch) {
  for (int i = 0; i < n; ++i) {
    const float x = xy[2 * i], y = xy[2 * i + 1];
    const int l = level[i];
    if (!std::isfinite(x) || !std::isfinite(y)) { set_error("%s: frame %d: keypoint %d is not finite", entry, k, i); return OSH_ERR_INVALID; }
    if (l < 0 || l >= n_levels) { set_error("%s: frame %d: keypoint %d: level %d outside [0, %d)", entry, k, i, l, n_levels); return OSH_ERR_INVALID; }
    // compared as floats first: a coordinate beyond the int range must not reach the conversion
    bool inside = x >= 0.f && y >= 0.f && x <= (float)OSH_FAST_MAX_SIDE && y <= (float)OSH_FAST_MAX_SIDE;
    if (inside) {
      const int cx = fast_cv_round(x), cy = fast_cv_round(y);
      inside = cx - R >= 0 && cx + R < lv[l].cols && cy - R >= 0 && cy + R < lv[l].rows;
    }
    if (!inside) { set_error("%s: frame %d: keypoint %d: the %d-pixel %s leaves level %d", entry, k, i, 2 * R + 1, patch, l); return OSH_ERR_INVALID; }
  }
  return OSH_OK;
}

// The levels of a call.  Frame: osh_ic_angle_frame or osh_describe_frame (pyramid, n_levels, pyramid_token, n and level under the
// same names).  In this order: check_brought, the entry's `no context` refusal, check_tokens, list.  check(k, n_levels, levels) is
// the entry's own validator of frame k.
template <class Frame>
struct PyramidLevels {
  const char* entry;
  int n_frames;
  const Frame* frames;
  bool any_token = false;              // after check_brought: a frame names the resident pyramid
  std::vector<PyramidLevel> lv;        // after list: every level of the call, frame after frame
  std::vector<int> level0, n_levels;   // of frame k: its first entry of lv, and how many
  size_t img_bytes = 0;                // the brought levels, packed one after another

  // The levels of frame k, off not yet set for a brought one; their number, 0: the frame's token names no frame of rp
  int levels_of(int k, const PyramidTable* rp, PyramidLevel* out) const {
    const Frame& f = frames[k];
    const FastFrameHost* F = f.pyramid ? nullptr : rp->frame(f.pyramid_token);
    for (int l = 0; f.pyramid && l < f.n_levels; ++l) out[l] = {false, 0, f.pyramid[l].rows, f.pyramid[l].cols};
    for (int l = 0; F && l < F->n_levels; ++l) { const FastLevelHost& L = rp->levels[F->level0 + l]; out[l] = {true, (size_t)L.img_off, L.rows, L.cols}; }
    return f.pyramid ? f.n_levels : F ? F->n_levels : 0;
  }
  // The frames that bring their pyramid: their refusals need no context and no device
  template <class Check>
  int check_brought(Check&& check) {
    PyramidLevel one[OSH_STEREO_MAX_LEVELS];
    for (int k = 0; k < n_frames; ++k) {
      if (!frames[k].pyramid) { any_token = true; continue; }
      OSH_TRY(fast_validate_pyramid(entry, k, frames[k].n_levels, frames[k].pyramid));
      OSH_TRY(check(k, levels_of(k, nullptr, one), one));
    }
    return OSH_OK;
  }
  // The frames that name the resident pyramid rp (not read when there is none)
  template <class Check>
  int check_tokens(const PyramidTable* rp, Check&& check) {
    PyramidLevel one[OSH_STEREO_MAX_LEVELS];
    for (int k = 0; k < n_frames; ++k) {
      if (frames[k].pyramid) continue;
      const int n = levels_of(k, rp, one);
      if (!n) { set_error("%s: frame %d: the token names no frame of this context's resident pyramid", entry, k); return OSH_ERR_INVALID; }
      OSH_TRY(check(k, n, one));
    }
    return OSH_OK;
  }
  // lv, level0, n_levels and img_bytes, of frames that passed the two checks
  int list(const PyramidTable* rp) {
    PyramidLevel one[OSH_STEREO_MAX_LEVELS];
    level0.resize(n_frames); n_levels.resize(n_frames);
    for (int k = 0; k < n_frames; ++k) {
      level0[k] = (int)lv.size(); n_levels[k] = levels_of(k, rp, one);
      for (int l = 0; l < n_levels[k]; ++l) {
        if (!one[l].resident) { one[l].off = img_bytes; img_bytes += (size_t)one[l].rows * one[l].cols; }
        lv.push_back(one[l]);
      }
      if (img_bytes > (size_t)1 << 31) { set_error("%s: batch too large", entry); return OSH_ERR_UNSUPPORTED; }
    }
    return OSH_OK;
  }
  // The brought levels into the img_bytes at `uploaded` (host staging), rows packed
  void stage(unsigned char* uploaded) const {
    for (int k = 0; k < n_frames; ++k)
      for (int l = 0; frames[k].pyramid && l < n_levels[k]; ++l) pack_level(uploaded + lv[level0[k] + l].off, frames[k].pyramid[l]);
  }
  // First pixel of level l on the device, given where the resident pyramid and the uploaded levels start there
  const unsigned char* data(size_t l, const unsigned char* resident, const unsigned char* uploaded) const {
    return (lv[l].resident ? resident : uploaded) + lv[l].off;
  }
  // Every keypoint's entry of lv, the keypoints of the frames one after another
  void index(int* dst) const {
    for (int k = 0; k < n_frames; ++k) {
      const int first = level0[k], n = frames[k].n;   // locals: dst may alias neither
      const int32_t* level = frames[k].level;
      for (int i = 0; i < n; ++i) dst[i] = first + level[i];
      dst += n;
    }
  }
};

}  // namespace osh
