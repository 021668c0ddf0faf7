// stereo_frame.h -- the host half of the rectified stereo matcher that its three entries share (stereo_device.hip):
// osh_orb_stereo_match (the caller brings both pyramids, the used levels are packed into the call's image arena and uploaded),
// osh_orb_stereo_match_resident (the pyramids are frames of the context's resident pyramid, named by token; nothing of them is
// staged) and the stereo tail of osh_orb_extract_stereo (the frames an extract has just built).  What is shared: the validator of
// keypoints, bf and b, the device frame descriptor and the plan of its level tables (sizes and byte offsets from one base pointer).
// Host code only: no kernel and no HIP call (`make stereo-frame-check` runs it in a plain host program).
#pragma once
#include "common.h"
#include "orb_pyramid_set.h"
#include "orb_stage.h"
#include <cmath>

namespace osh {

struct StereoFrameDev {
  int n_left, n_right, left_base, right_base;   // bases: offsets of this frame in the keypoint arrays of the batch
  int n_rows;                                   // mvImagePyramid[0].rows of the left extractor
  int n_levels;
  float bf, b;
  float sf[OSH_STEREO_MAX_LEVELS], isf[OSH_STEREO_MAX_LEVELS];
  int rows_l[OSH_STEREO_MAX_LEVELS], cols_l[OSH_STEREO_MAX_LEVELS], rows_r[OSH_STEREO_MAX_LEVELS], cols_r[OSH_STEREO_MAX_LEVELS];
  long long off_l[OSH_STEREO_MAX_LEVELS], off_r[OSH_STEREO_MAX_LEVELS];   // byte offsets from the image base (rows packed, stride = cols); -1: not there
};

// The levels of osh_stereo_frame: brought along by the caller
struct BroughtStereoLevels {
  static bool present(const osh_stereo_frame& f) { return f.left_pyramid && f.right_pyramid; }
  static int rows0(const osh_stereo_frame& f) { return f.left_pyramid[0].rows; }
  // The side (0 left, 1 right) whose level o cannot be read; -1: both can
  static int unreadable(const osh_stereo_frame& f, int o) {
    const osh_stereo_image* im[2] = {&f.left_pyramid[o], &f.right_pyramid[o]};
    for (int s = 0; s < 2; ++s)
      if (!im[s]->data || im[s]->rows <= 0 || im[s]->cols <= 0 || im[s]->stride < im[s]->cols) return s;
    return -1;
  }
};
// The levels of osh_stereo_resident_frame: frames of a resident pyramid, which holds no level that cannot be read
struct ResidentStereoLevels {
  static bool present(const osh_stereo_resident_frame&) { return true; }
  static int rows0(const osh_stereo_resident_frame&) { return 1; }
  static int unreadable(const osh_stereo_resident_frame&, int) { return -1; }
};

// What every entry refuses of the keypoints, bf and b of frame k, and of the levels the caller brings
template <class Levels, class Frame>
int stereo_validate_frame(int k, const Frame& f, const osh_stereo_result& r, unsigned pos_mask) {
  if (f.n_left < 0 || f.n_right < 0) { set_error("frame %d: negative keypoint count", k); return OSH_ERR_INVALID; }
  OSH_TRY(validate_keypoint_sides(k, f, pos_mask));
  if (!f.scale_factors || !f.inv_scale_factors || !Levels::present(f)) { set_error("frame %d: NULL scale factors or pyramid", k); return OSH_ERR_INVALID; }
  if (f.n_left && (!f.left_xy || !f.left_octave || !f.left_desc || !r.u_right || !r.depth)) { set_error("frame %d: NULL left keypoint or result array", k); return OSH_ERR_INVALID; }
  if (f.n_right && (!f.right_xy || !f.right_octave || !f.right_desc)) { set_error("frame %d: NULL right keypoint array", k); return OSH_ERR_INVALID; }
  if (!(f.b > 0.f) || !std::isfinite(f.bf) || !std::isfinite(f.b)) { set_error("frame %d: bad bf / b", k); return OSH_ERR_INVALID; }
  if (Levels::rows0(f) <= 0) { set_error("frame %d: left_pyramid[0].rows must be positive", k); return OSH_ERR_INVALID; }
  auto coords_ok = [](const float* xy, int n) {
    for (int i = 0; i < 2 * n; ++i) if (!(std::fabs(xy[i]) <= OSH_STEREO_MAX_COORD)) return false;   // NaN fails too
    return true;
  };
  if (!coords_ok(f.left_xy, f.n_left) || !coords_ok(f.right_xy, f.n_right)) { set_error("frame %d: keypoint coordinate not finite or beyond %g", k, (double)OSH_STEREO_MAX_COORD); return OSH_ERR_INVALID; }
  OSH_TRY(validate_octaves(k, "right", f.right_octave, f.n_right, f.n_levels));
  for (int i = 0; i < f.n_left; ++i) {   // octave and image keypoint by keypoint: not validate_octaves, which would test every octave first
    const int o = f.left_octave[i];
    if (o < 0 || o >= f.n_levels) { set_error("frame %d: left octave %d outside [0, %d)", k, o, f.n_levels); return OSH_ERR_INVALID; }
    const int side = Levels::unreadable(f, o);
    if (side >= 0) {
      set_error("frame %d: level %d (%s) is used by a left keypoint but its image is NULL, empty or has stride < cols", k, o, side ? "right" : "left");
      return OSH_ERR_INVALID;
    }
  }
  return OSH_OK;
}

// The counts, bases, bf, b and scale tables of a device frame; its level tables are the plans' below
inline StereoFrameDev stereo_frame_dev(int n_left, int n_right, int left_base, int right_base, int n_levels, float bf, float b, const float* sf, const float* isf) {
  StereoFrameDev d;
  std::memset(&d, 0, sizeof d);
  d.n_left = n_left; d.n_right = n_right; d.left_base = left_base; d.right_base = right_base;
  d.n_levels = n_levels; d.bf = bf; d.b = b;
  for (int l = 0; l < OSH_STEREO_MAX_LEVELS; ++l) { d.off_l[l] = d.off_r[l] = -1; d.sf[l] = d.isf[l] = 1.f; }
  for (int l = 0; l < n_levels; ++l) { d.sf[l] = sf[l]; d.isf[l] = isf[l]; }
  return d;
}

// Brought levels: the sizes of every level, and the levels a left keypoint names packed one after another (left, then right) into
// an arena that grows by them
inline void stereo_plan_brought(const osh_stereo_frame& f, StereoFrameDev& d, size_t& img_bytes) {
  bool used[OSH_STEREO_MAX_LEVELS] = {false};
  for (int i = 0; i < f.n_left; ++i) used[f.left_octave[i]] = true;
  d.n_rows = f.left_pyramid[0].rows;
  for (int l = 0; l < f.n_levels; ++l) {
    d.rows_l[l] = f.left_pyramid[l].rows; d.cols_l[l] = f.left_pyramid[l].cols;
    d.rows_r[l] = f.right_pyramid[l].rows; d.cols_r[l] = f.right_pyramid[l].cols;
    if (!used[l]) continue;
    d.off_l[l] = (long long)img_bytes; img_bytes += (size_t)d.rows_l[l] * d.cols_l[l];
    d.off_r[l] = (long long)img_bytes; img_bytes += (size_t)d.rows_r[l] * d.cols_r[l];
  }
}

// Resident levels: the two frames of the table as they lie in the resident pyramid, offsets from its first byte
inline void stereo_plan_resident(const PyramidTable& t, const FastFrameHost& L, const FastFrameHost& R, StereoFrameDev& d) {
  d.n_rows = t.levels[L.level0].rows;
  for (int l = 0; l < L.n_levels && l < R.n_levels && l < OSH_STEREO_MAX_LEVELS; ++l) {
    const FastLevelHost& a = t.levels[L.level0 + l];
    const FastLevelHost& b = t.levels[R.level0 + l];
    d.rows_l[l] = a.rows; d.cols_l[l] = a.cols; d.off_l[l] = a.img_off;
    d.rows_r[l] = b.rows; d.cols_r[l] = b.cols; d.off_r[l] = b.img_off;
  }
}

// The row lists of the search that the entries on resident pyramids run (k_stereo_rows_*, k_stereo_rowsearch of stereo_device.hip):
// of a frame its first row in the per-row arrays of the batch and its slice [entry0, entry_end) of the entries
struct StereoRowsDev { int row0, entry0, entry_end; };
constexpr size_t kStereoMaxRows = (size_t)1 << 24, kStereoMaxRowEntries = (size_t)1 << 26;
struct StereoRowPlan {
  std::vector<StereoRowsDev> frames;
  size_t rows = 0, entries = 0;
  bool too_large = false;
  // A frame's slice holds every entry its right keypoints can make: a keypoint enters rows floor(y - r) .. ceil(y + r), r = 2 sf,
  // evaluated in float32 on |y| <= OSH_STEREO_MAX_COORD: at most 2 r + 3.5 rows, and never more than the n_rows they are clipped to
  void add(const StereoFrameDev& d) {
    float sf_max = 0.f;
    for (int l = 0; l < d.n_levels; ++l) sf_max = d.sf[l] > sf_max || d.sf[l] != d.sf[l] ? d.sf[l] : sf_max;
    const double span = 4.0 * (double)sf_max + 4.0;
    const size_t per = span < (double)d.n_rows ? (size_t)span : (size_t)std::max(d.n_rows, 0);   // NaN: n_rows
    const size_t cap = (size_t)d.n_right * per;
    const size_t n_rows = (size_t)std::max(d.n_rows, 0);
    if (rows + n_rows > kStereoMaxRows || entries + cap > kStereoMaxRowEntries) too_large = true;
    if (too_large) { frames.push_back({0, 0, 0}); return; }
    frames.push_back({(int)rows, (int)entries, (int)(entries + cap)});
    rows += n_rows; entries += cap;
  }
  // Beyond these sizes the entries launch k_stereo_hamming instead
  bool fits() const { return !too_large; }
};

// The two tokens of frame k against the table (nullptr: the context has no resident pyramid) and the frame's n_levels
inline int stereo_check_tokens(const char* entry, int k, const PyramidTable* t, uint64_t left_token, uint64_t right_token, int n_levels,
                               const FastFrameHost** L, const FastFrameHost** R) {
  *L = t ? t->frame(left_token) : nullptr;
  *R = t ? t->frame(right_token) : nullptr;
  if (!*L || !*R) { set_error("%s: frame %d: the token names no frame of this context's resident pyramid", entry, k); return OSH_ERR_INVALID; }
  if ((*L)->n_levels != (*R)->n_levels || (*L)->n_levels != n_levels) {
    set_error("%s: frame %d: the left frame has %d levels, the right frame %d, the call names %d", entry, k, (*L)->n_levels, (*R)->n_levels, n_levels);
    return OSH_ERR_INVALID;
  }
  return OSH_OK;
}

}  // namespace osh
