// orb_extract.h -- what osh_orb_extract (orb_extract_device.hip) shares with the translation units of its stages.  Every stage of
// ORBextractor::operator() has ONE form that works on device-resident keypoints, and both the stage's own entry and the fused call
// go through it: fast_emit (orb_fast_device.hip) leaves the candidates where k_fast_emit wrote them, octree_run
// (orb_octree_device.hip) reads candidates and leaves the kept indices on the device, ic_angle_launch and brief_launch
// (orb_fast_device.hip, orb_brief_device.hip) read keypoint arrays on the device.  The stage entries stage host arrays into those
// forms and download what they leave; the fused call chains them.  A tail (ExtractTail below) may follow the descriptors on the same
// stream and add its outputs to the one download: the stereo match of osh_orb_extract_stereo (stereo_device.hip).
#pragma once
#include "common.h"
#include "orb_pyramid_set.h"
#include <functional>
#include <vector>

namespace osh {

// ---- orb_fast_device.hip
struct EmittedLevel { int rows, cols; long long img_off; int key0, n; };   // a level of the resident pyramid and its candidates [key0, key0 + n)
struct FastEmitted {
  std::vector<EmittedLevel> levels;   // of every frame of the call, frame after frame
  std::vector<int> level0;            // [n_frames + 1] first level of frame k
  const unsigned char* images;        // device: first byte of the resident pyramid
  const float2* xy;                   // device: pt relative to minBorder; nullptr when the call has no candidate
  const float* response;
};
// The detector over frames of the resident pyramid (tokens as osh_orb_fast_detect_resident), nothing downloaded but the cell offsets
int fast_emit_resident(const char* entry, osh_orb_ctx* c, hipStream_t s, int n_frames, const osh_fast_resident_frame* frames, FastEmitted& e);
int ic_angle_launch(hipStream_t s, int n, const PyramidLevelDev* levels, const int* level_index, const float2* xy, float* angle, int* m10, int* m01);

// ---- orb_pyramid_device.hip
// Where the level 0 of every frame of a build comes from when it is not a host image: a device producer (orb_prepare_device.hip)
struct Level0Producer {
  // the refusals that need the context's device; called before the resident pyramid is touched
  std::function<int(int device)> check;
  // on the stream, before k_pyr_level: level 0 of frame k (rows packed at `cols` bytes) to images + level0_off[k]
  std::function<int(hipStream_t s, unsigned char* images, const std::vector<long long>& level0_off)> produce;
};
// osh_orb_pyramid_build with level 0 from the host images (producer == nullptr) or from a device producer (frames[k].image then
// carries the size and no data).  Refusals, tokens and outputs are osh_orb_pyramid_build's.
int pyramid_build_from(osh_orb_ctx* c, int32_t n_frames, const osh_pyramid_frame* frames, osh_pyramid_result* results, const Level0Producer* producer);

// ---- orb_extract_device.hip
// What a tail of the fused call sees once the descriptors are launched: the kept keypoints of the call on the device, frame k's at
// [frame_kp0[k], frame_kp0[k] + frame_n[k]) in level-then-list order, and the level tables of the call
struct ExtractKept {
  size_t K;                               // keypoints of the call
  const float2* xy;                       // device [K] in the pixels of their level
  const int* level_index;                 // device [K] the keypoint's entry of e->levels
  const unsigned long long* desc;         // device [K * 4], 256-byte aligned: the 32 bytes of keypoint i at desc + 4 i
  const unsigned char* images;            // device: first byte of the resident pyramid
};
// A stage that runs after brief_launch and before the one download of extract_from (the stereo match of osh_orb_extract_stereo).
// With no tail the call launches and downloads what it did without the hook.
struct ExtractTail {
  // The frames in the order their keypoints are laid out on the device (a permutation of 0 .. n_frames - 1)
  std::vector<int> order;
  // On the host, the counts known: the tail's sections of the call's three layouts (`out` comes down with the results)
  std::function<int(const FastEmitted& e, const std::vector<size_t>& frame_kp0, const std::vector<size_t>& frame_n, Layout& in, Layout& out, Layout& work)> plan;
  std::function<void(char* host_in)> stage;   // its inputs into the staging buffer
  std::function<int(hipStream_t s, char* dev_in, char* dev_out, char* dev_work, const ExtractKept& kept)> launch;
  std::function<void(const char* host_out)> collect;   // after the download; not called when the call kept no keypoint
};
// osh_orb_extract with the pyramid built by pyramid_build_from(.., producer) and an optional tail
int extract_from(const char* entry, osh_orb_ctx* c, int32_t n_frames, const osh_extract_frame* frames, osh_extract_result* results, const Level0Producer* producer,
                 const ExtractTail* tail = nullptr);

// ---- orb_prepare_device.hip
// The body of osh_orb_extract_raw: extract_from with the device producer of level 0, then the prepared images (prepare_results may be NULL)
int extract_raw_from(const char* entry, osh_orb_ctx* c, int32_t n_frames, const osh_prepare_frame* prepare_frames, const osh_extract_frame* extract_frames,
                     osh_extract_result* extract_results, osh_prepare_result* prepare_results, const ExtractTail* tail);

// ---- orb_octree_device.hip
struct OctListDev {
  int key0;        // first candidate in xy / response
  int n, W, H, N;
  int out0;        // first entry in the kept indices; the list may write min(n, kOctMaxNodes)
  long long work0; // first entry in the key buffers (2 n of them) when n is beyond the kernel's LDS
};
// k_octree on `lists` (out0 and work0 are filled here) over candidates on the device.  count and status come back per list; the kept
// indices stay on the device at *index, list k's from lists[k].out0, until the context's next octree run.
int octree_run(osh_orb_ctx* c, hipStream_t s, std::vector<OctListDev>& lists, const float2* xy, const float* response, std::vector<int>& count,
               std::vector<int>& status, const int** index);

// ---- orb_brief_device.hip
struct BlurLevelDev {
  const unsigned char* src;    // first pixel of the packed level
  unsigned char* dst;          // of the blurred level
  int rows, cols;
  unsigned short w[8];         // w[0..6]
};
struct BlurTileDev { int level, tx, ty; };
struct BriefView {
  int n;
  const PyramidLevelDev* levels;   // the blurred levels of every frame of the call, frame after frame
  const int* level_index;          // [n] the keypoint's entry of `levels`
  const int* frame;                // [n] the keypoint's frame: its table
  const float2* xy;                // [n]
  const float* angle;              // [n]
  const signed char* pattern;      // [n_frames * 1024]
  unsigned long long* desc;        // [n * 4]
  float2* cos_sin;                 // [n]
};
// Entry l of a call's blur plan (w == nullptr: the default weights), and its tiles
BlurLevelDev blur_level(const unsigned char* src, unsigned char* dst, int rows, int cols, const uint16_t* w);
void blur_tiles(int l, int rows, int cols, std::vector<BlurTileDev>& tiles);
// The context's arena of blurred levels, at least `bytes` long; nullptr: the allocation failed (osh_last_error says why)
unsigned char* brief_blurred(osh_orb_ctx* c, size_t bytes);
// k_orb_blur over the tiles, then k_orb_brief over v.n keypoints; blur, tiles and everything v names are on the device
int brief_launch(hipStream_t s, size_t n_tiles, const BlurLevelDev* blur, const BlurTileDev* tiles, const BriefView& v);

}  // namespace osh
