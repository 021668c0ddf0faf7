// mappoint_refresh.h -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403) and MapPoint::UpdateNormalAndDepth
// (:426-494) for one map point, given its entries in observation order.  An entry is one camera of one observing keyframe: a
// 32-byte descriptor, the index of a camera centre and the flag use_desc, which is 0 when the keyframe is bad (the reference skips
// bad keyframes for the descriptor, :352, but not for the normal, :447-466).  Device code of mappoint_device.hip; plain C++ as
// well, so the test library and MapPoint::RefreshBatch can run the same statements on the host.
//
// Descriptor: over the M entries with use_desc, in order, d(i, j) is the Hamming distance, the median of row i is the element of
// index (M - 1) / 2 of the ascending row (self-distance 0 included: vDists[0.5 * (N - 1)], :390), and the result is the first row
// with the least median (strict <, :392).  The reference's float Distances[N][N] holds integers up to 256: an integer table is the
// same thing.  M = 0: index -1 and median -1, and the caller leaves the descriptor alone.
//
// Normal and depth: float32, every operation rounded, contraction off.  normali = Pos - Ow; the norm is sqrt(x*x + (y*y + z*z))
// (the order this project uses for a Vector3f norm, csrc/host/LocalMapping.cc); normal += normali / norm component-wise by true
// division, one sequential chain over all entries in observation order; mNormalVector = normal / (float)n; dist is the norm of
// Pos - Ow_ref (the left centre of the reference keyframe); mfMaxDistance = dist * levelScaleFactor and mfMinDistance =
// mfMaxDistance / mvScaleFactors[nLevels - 1].  sqrt is the FP64 function rounded once (correctly rounded, as kb8_sqrt), `/` is the
// correctly rounded float32 division on both sides.  Parity with the code Eigen generates for these statements is not pinned.
#pragma once
#include <cstdint>
#include "kb8_triangulate.h"

namespace osh {

struct MpPoint {          // one map point of a packed call
  int entry_base, n;      // its entries in the arrays of the call
  float pos[3];           // mWorldPos
  int ref_centre;         // the left centre of mpRefKF in the centre table
  float level_scale;      // pRefKF->mvScaleFactors[level]
  float top_scale;        // pRefKF->mvScaleFactors[nLevels - 1]
};
struct MpOut {
  int best_entry, best_median;
  float normal[3], min_distance, max_distance;
};

// the index of the median in an ascending row of M distances (:390)
OSH_KB8_HD int mp_median_index(int M) { return (M - 1) / 2; }

OSH_KB8_HD int mp_hamming(const uint32_t* a, const uint32_t* b) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// normali / normali.norm() (:456-457)
OSH_KB8_HD void mp_unit_vector(const float pos[3], const float* ow, float u[3]) {
#pragma clang fp contract(off)
  const float x = pos[0] - ow[0], y = pos[1] - ow[1], z = pos[2] - ow[2];
  const float norm = kb8_sqrt(kb8_sum3(x * x, y * y, z * z));
  u[0] = x / norm; u[1] = y / norm; u[2] = z / norm;
}

// :468-492 from the finished sum of the n unit vectors
OSH_KB8_HD void mp_finish(const MpPoint& p, const float sum[3], const float* ow_ref, MpOut& o) {
#pragma clang fp contract(off)
  const float fn = (float)p.n;
  o.normal[0] = sum[0] / fn; o.normal[1] = sum[1] / fn; o.normal[2] = sum[2] / fn;
  const float x = p.pos[0] - ow_ref[0], y = p.pos[1] - ow_ref[1], z = p.pos[2] - ow_ref[2];
  const float dist = kb8_sqrt(kb8_sum3(x * x, y * y, z * z));
  o.max_distance = dist * p.level_scale;
  o.min_distance = o.max_distance / p.top_scale;
}

// a point without entries: nothing to apply
OSH_KB8_HD void mp_empty(MpOut& o) {
  o.best_entry = -1; o.best_median = -1;
  o.normal[0] = o.normal[1] = o.normal[2] = 0.f; o.min_distance = o.max_distance = 0.f;
}

// One point on one thread: what the host build runs.  desc: 8 words per entry; centre: index into centres (3 floats each);
// use_desc: one byte per entry, all three indexed from the point's first entry.  The median of a row comes from the counts of its
// distances (257 bins), walked up to the median's rank; `table` needs room for n * n distances (each pair is computed once, as in
// the reference).
inline void mappoint_refresh_point(const MpPoint& p, const uint32_t* desc, const int32_t* centre, const uint8_t* use_desc, const float* centres,
                                   uint16_t* table, MpOut& o) {
#pragma clang fp contract(off)
  if (p.n <= 0) { mp_empty(o); return; }
  const int n = p.n;
  int M = 0;
  for (int i = 0; i < n; ++i) M += use_desc[i] != 0;
  o.best_entry = -1; o.best_median = -1;
  if (M > 0) {
    for (int i = 0; i < n; ++i) {
      if (!use_desc[i]) continue;
      table[(size_t)i * n + i] = 0;
      for (int j = i + 1; j < n; ++j) {
        if (!use_desc[j]) continue;
        const uint16_t d = (uint16_t)mp_hamming(desc + 8 * (size_t)i, desc + 8 * (size_t)j);
        table[(size_t)i * n + j] = d; table[(size_t)j * n + i] = d;
      }
    }
    const int rank = mp_median_index(M);
    int best = 0x7fffffff;
    for (int i = 0; i < n; ++i) {
      if (!use_desc[i]) continue;
      uint16_t count[257] = {0};
      for (int j = 0; j < n; ++j) if (use_desc[j]) ++count[table[(size_t)i * n + j]];
      int median = 0, below = count[0];
      while (below <= rank) below += count[++median];
      if (median < best) { best = median; o.best_entry = i; }
    }
    o.best_median = best;
  }
  float sum[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < n; ++i) {
    float u[3];
    mp_unit_vector(p.pos, centres + 3 * (size_t)centre[i], u);
    sum[0] = sum[0] + u[0]; sum[1] = sum[1] + u[1]; sum[2] = sum[2] + u[2];
  }
  mp_finish(p, sum, centres + 3 * (size_t)p.ref_centre, o);
}

}  // namespace osh
