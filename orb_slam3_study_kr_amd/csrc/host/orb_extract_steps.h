// orb_extract_steps.h -- the steps of csrc/host/ORBextractor.cc that make no device call, each stated once for the bodies that need
// it: the size of a pyramid level (ComputePyramid, ExtractBatch), `pattern` as the table of the calls (operator(), ExtractBatch) and
// the write-back of reference src/ORBextractor.cc:1120-1167 (operator(), ExtractBatch).  Nothing here names OpenCV or HIP: the
// keypoint and point types are the caller's, so `make extractor-host-check` runs the steps on exactly-sized arrays under the sanitizers.
// An integrator copies this file with ORBextractor.cc.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace ORB_SLAM3 {

constexpr int kEdge = 19;   // EDGE_THRESHOLD: the border around every level of mvImagePyramid

// rows x cols of a level (:1174-1175): cvRound of the float product.  False: the level has no pixels or too many
inline bool LevelShape(int rows, int cols, float invScale, int& h, int& w) {
  const float fw = (float)cols * invScale, fh = (float)rows * invScale;
  w = fw >= 0.f && fw < 1.0e6f ? (int)std::nearbyint(fw) : 0;
  h = fh >= 0.f && fh < 1.0e6f ? (int)std::nearbyint(fh) : 0;
  return w > 0 && h > 0;
}

// rows x cols of the grey image ExtractBatchRaw extracts from, as osh_orb_prepare sizes it: the size asked for (newImSize) when there
// is one, else the rectification map's when there is a map (mapRows > 0), else the raw image's
inline void PreparedShape(int rawRows, int rawCols, int mapRows, int mapCols, int newRows, int newCols, int& h, int& w) {
  if (newRows != 0 || newCols != 0) { h = newRows; w = newCols; }
  else if (mapRows > 0) { h = mapRows; w = mapCols; }
  else { h = rawRows; w = rawCols; }
}

// The 512 points of `pattern` as the int8 table [1024] of osh_orb_describe and osh_orb_extract, x and y interleaved.  False: a
// coordinate does not fit 8 bits (the table is filled all the same)
template <class Point>
inline bool PatternTable(const Point* pattern, int8_t* table) {
  bool fits = true;
  for (int i = 0; i < 512; ++i) {
    fits = fits && pattern[i].x >= -128 && pattern[i].x <= 127 && pattern[i].y >= -128 && pattern[i].y <= 127;
    table[2 * i] = (int8_t)pattern[i].x; table[2 * i + 1] = (int8_t)pattern[i].y;
  }
  return fits;
}

// :1120-1167 for n keypoints, one call per keypoint in the order of the descriptor rows: the keypoint (level pixels, the level in
// `octave`) is scaled to level 0 and goes with its descriptor [32] to the back of `out` [n] and of the rows of `outDesc` (`outStep`
// bytes apart) if it lies in the lapping area, to the front if not.  monoIndex after the last call is what operator() returns
template <class KeyPoint>
struct WriteBack {
  const float* scaleFactor; const int* lapping;
  KeyPoint* out; uint8_t* outDesc; size_t outStep;
  int monoIndex, stereoIndex;
  WriteBack(int n, const float* scaleFactor_, const int* lapping_, KeyPoint* out_, uint8_t* outDesc_, size_t outStep_)
      : scaleFactor(scaleFactor_), lapping(lapping_), out(out_), outDesc(outDesc_), outStep(outStep_), monoIndex(0), stereoIndex(n - 1) {}
  void operator()(KeyPoint keypoint, const uint8_t* desc) {
    if (keypoint.octave != 0) keypoint.pt *= scaleFactor[keypoint.octave];
    const int at = keypoint.pt.x >= lapping[0] && keypoint.pt.x <= lapping[1] ? stereoIndex-- : monoIndex++;
    out[at] = keypoint;
    std::memcpy(outDesc + (size_t)at * outStep, desc, 32);
  }
};

}  // namespace ORB_SLAM3
