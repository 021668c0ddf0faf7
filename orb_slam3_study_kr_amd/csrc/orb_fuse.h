// orb_fuse.h -- what both ORBmatcher::Fuse overloads (src/ORBmatcher.cc:1196-1290 and :1368-1434) compute for ONE (target keyframe,
// map point) pair before their loops touch the map: the projection with its gates, MapPoint::PredictScale, the window of
// KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:704-745) and the candidate scan.  Device code of orb_fuse_device.hip; plain C++ as
// well, so the test library, `make fuse-check` and the replay of a stale point run the same statements on the host.
//
// Float32 throughout like the reference, every operation rounded once, contraction off; Eigen's three-term reductions are
// a0 + (a1 + a2) and sqrt, atan2, cos, sin and log are the FP64 function rounded once, as in k_frustum (orb_device.hip).  A float
// that no int holds converts to INT_MIN in the reference's build (cvttss2si): fuse_level and fuse_cell state that outcome instead
// of the conversion, which C++ leaves undefined.
#pragma once
#include <cstdint>
#include "../../include/orbslam3_hip.h"
#include "kb8_triangulate.h"

namespace osh {

struct FuseTarget {               // one target of a packed call: osh_fuse_target with its arrays as offsets
  float R[9], t[3], O[3];
  float fx, fy, cx, cy, kb[4], bf;
  float min_x, max_x, min_y, max_y;
  float grid_min_x, grid_min_y, winv, hinv;
  int cols, rows;
  int camera, n_levels;
  float log_sf, th;
  float scale[OSH_FUSE_MAX_LEVELS], inv_sigma2[OSH_FUSE_MAX_LEVELS];
  int key_base, n_keys;           // its keypoints in the concatenated keypoint arrays
  int cell_base;                  // its cols * rows + 1 cell offsets in the concatenated offset array (entries relative to key_base)
  int has_uright;
};

// the scalar fields of a valid osh_fuse_target; the offsets are the caller's
inline void fuse_fill_target(const osh_fuse_target& s, FuseTarget& T) {
  for (int k = 0; k < 9; ++k) T.R[k] = s.Rcw[k];
  for (int k = 0; k < 3; ++k) { T.t[k] = s.tcw[k]; T.O[k] = s.Ow[k]; }
  T.fx = s.fx; T.fy = s.fy; T.cx = s.cx; T.cy = s.cy; T.bf = s.bf;
  for (int k = 0; k < 4; ++k) T.kb[k] = s.camera == OSH_FUSE_KB8 ? s.kb8[k] : 0.f;
  T.min_x = s.min_x; T.max_x = s.max_x; T.min_y = s.min_y; T.max_y = s.max_y;
  T.grid_min_x = s.grid_min_x; T.grid_min_y = s.grid_min_y; T.winv = s.cell_w_inv; T.hinv = s.cell_h_inv;
  T.cols = s.cols; T.rows = s.rows; T.camera = s.camera; T.n_levels = s.n_levels; T.log_sf = s.log_scale_factor; T.th = s.th;
  for (int k = 0; k < OSH_FUSE_MAX_LEVELS; ++k) {
    T.scale[k] = k < s.n_levels ? s.scale_factors[k] : 0.f;
    T.inv_sigma2[k] = k < s.n_levels ? s.inv_level_sigma2[k] : 0.f;
  }
  T.key_base = 0; T.n_keys = s.n_keys; T.cell_base = 0; T.has_uright = s.key_uright != nullptr;
}

struct FuseGeom {                 // the geometric outputs of a pair
  int stage;
  float u, v, ur;
  int level;
  float radius;
};

struct FuseWindow { int x0, y0, nx, ny; };   // cells [x0, x0 + nx) x [y0, y0 + ny); nx * ny == 0: none

// the keypoints of one target
struct FuseKeys {
  const float* xy; const int* octave; const float* uright; const uint32_t* desc;   // at the target's first keypoint
  const int* cell_off; const int* cell_idx;                                          // cell_idx holds indices among the target's keypoints
};

OSH_KB8_HD int fuse_hamming(const uint32_t* a, const uint32_t* b) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// MapPoint::PredictScale (src/MapPoint.cc:531-546) for a keyframe
OSH_KB8_HD int fuse_level(float max_dist, float dist, float log_sf, int n_levels) {
#pragma clang fp contract(off)
  const float ratio = max_dist / dist;
  const float lg = (float)log((double)ratio);
  const float f = ceilf(lg / log_sf);
  if (!(f >= 0.f) || f >= 2147483648.f) return 0;   // negative; NaN or beyond int: INT_MIN, clamped to 0
  return f >= (float)n_levels ? n_levels - 1 : (int)f;
}

// (int)floor(f) / (int)ceil(f) where only the comparison with [0, cells) matters: any value below 0 as -1, any value from the limit up
// as the limit -- except what no int holds (NaN, +-2^31 and beyond), which is INT_MIN in the reference's build and so -1 as well: a
// radius that overflows the conversion ends in an early return there, not in a window over the whole grid
OSH_KB8_HD int fuse_cell(float f) {
  if (!(f > -1.f) || f >= 2147483648.f) return -1;
  return f >= (float)OSH_FUSE_MAX_CELLS ? OSH_FUSE_MAX_CELLS : (int)f;
}

// Everything up to the window: stage is one of SKIPPED .. ANGLE, or SEARCHED for a pair that goes on to fuse_window / fuse_scan
OSH_KB8_HD void fuse_project(const FuseTarget& T, const float* P, const float* Pn, float min_dist, float max_dist, bool skip, FuseGeom& g) {
#pragma clang fp contract(off)
  g.stage = OSH_FUSE_SKIPPED; g.u = 0.f; g.v = 0.f; g.ur = 0.f; g.level = -1; g.radius = 0.f;
  if (skip) return;
  float Pc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) Pc[r] = kb8_sum3(T.R[3 * r] * P[0], T.R[3 * r + 1] * P[1], T.R[3 * r + 2] * P[2]) + T.t[r];
  g.stage = OSH_FUSE_BEHIND;
  if (Pc[2] < 0.0f) return;
  const float invz = 1.0f / Pc[2];
  float uv[2];
  if (T.camera == OSH_FUSE_KB8) {
    const float cam[8] = {T.fx, T.fy, T.cx, T.cy, T.kb[0], T.kb[1], T.kb[2], T.kb[3]};
    kb8_project(cam, Pc, uv);                           // src/CameraModels/KannalaBrandt8.cpp:67-84
  } else {
    uv[0] = T.fx * Pc[0] / Pc[2] + T.cx;                // Pinhole::project(Vector3f), src/CameraModels/Pinhole.cpp:43-49
    uv[1] = T.fy * Pc[1] / Pc[2] + T.cy;
  }
  g.stage = OSH_FUSE_OUTSIDE;
  if (!(uv[0] >= T.min_x && uv[0] < T.max_x && uv[1] >= T.min_y && uv[1] < T.max_y)) return;   // KeyFrame::IsInImage
  g.u = uv[0]; g.v = uv[1]; g.ur = uv[0] - T.bf * invz;
  const float PO[3] = {P[0] - T.O[0], P[1] - T.O[1], P[2] - T.O[2]};
  const float dist = kb8_sqrt(kb8_sum3(PO[0] * PO[0], PO[1] * PO[1], PO[2] * PO[2]));
  g.stage = OSH_FUSE_DISTANCE;
  if (dist < 0.8f * min_dist || dist > 1.2f * max_dist) return;   // GetMinDistanceInvariance / GetMaxDistanceInvariance
  g.stage = OSH_FUSE_ANGLE;
  if ((double)kb8_sum3(PO[0] * Pn[0], PO[1] * Pn[1], PO[2] * Pn[2]) < 0.5 * (double)dist) return;
  g.level = fuse_level(max_dist, dist, T.log_sf, T.n_levels);
  g.radius = T.th * T.scale[g.level];
  g.stage = OSH_FUSE_SEARCHED;
}

// The cell range of KeyFrame::GetFeaturesInArea with its four early returns
OSH_KB8_HD FuseWindow fuse_window(const FuseTarget& T, float x, float y, float r) {
#pragma clang fp contract(off)
  FuseWindow w = {0, 0, 0, 0};
  int v = fuse_cell(floorf((x - T.grid_min_x - r) * T.winv));
  const int nMinCellX = v > 0 ? v : 0;
  if (nMinCellX >= T.cols) return w;
  v = fuse_cell(ceilf((x - T.grid_min_x + r) * T.winv));
  const int nMaxCellX = v < T.cols - 1 ? v : T.cols - 1;
  if (nMaxCellX < 0) return w;
  v = fuse_cell(floorf((y - T.grid_min_y - r) * T.hinv));
  const int nMinCellY = v > 0 ? v : 0;
  if (nMinCellY >= T.rows) return w;
  v = fuse_cell(ceilf((y - T.grid_min_y + r) * T.hinv));
  const int nMaxCellY = v < T.rows - 1 ? v : T.rows - 1;
  if (nMaxCellY < 0) return w;
  if (nMaxCellX < nMinCellX || nMaxCellY < nMinCellY) return w;   // the reference's loops run no cell
  w.x0 = nMinCellX; w.y0 = nMinCellY; w.nx = nMaxCellX - nMinCellX + 1; w.ny = nMaxCellY - nMinCellY + 1;
  return w;
}

// One keypoint of the window: 0 not within the radius (not in vIndices), 1 in vIndices but no candidate, 2 a candidate
OSH_KB8_HD int fuse_candidate(const FuseTarget& T, const FuseKeys& K, int idx, const FuseGeom& g, int mode) {
#pragma clang fp contract(off)
  const float kx = K.xy[2 * idx], ky = K.xy[2 * idx + 1];
  const float distx = kx - g.u, disty = ky - g.v;
  if (!(fabsf(distx) < g.radius && fabsf(disty) < g.radius)) return 0;
  const int oct = K.octave[idx];
  if (oct < g.level - 1 || oct > g.level) return 1;
  if (mode == OSH_FUSE_CHI2) {
    const float ex = g.u - kx, ey = g.v - ky;
    const float kur = T.has_uright ? K.uright[idx] : -1.f;
    if (kur >= 0.f) {
      const float er = g.ur - kur;
      const float e2 = ex * ex + ey * ey + er * er;
      if ((double)(e2 * T.inv_sigma2[oct]) > 7.8) return 1;
    } else {
      const float e2 = ex * ex + ey * ey;
      if ((double)(e2 * T.inv_sigma2[oct]) > 5.99) return 1;
    }
  }
  return 2;
}

struct FuseFound { int n_in, n_candidates, best_idx, best_dist; };

// The reference's scan of a pair that passed fuse_project: ix-major, then iy, then insertion order; strict <, so the first least wins
OSH_KB8_HD FuseFound fuse_scan(const FuseTarget& T, const FuseKeys& K, const FuseGeom& g, const uint32_t* qdesc, int mode) {
  FuseFound f = {0, 0, -1, 256};
  const FuseWindow w = fuse_window(T, g.u, g.v, g.radius);
  for (int ix = w.x0; ix < w.x0 + w.nx; ++ix)
    for (int iy = w.y0; iy < w.y0 + w.ny; ++iy) {
      const int cell = ix * T.rows + iy;
      for (int k = K.cell_off[cell]; k < K.cell_off[cell + 1]; ++k) {
        const int idx = K.cell_idx[k];
        const int kind = fuse_candidate(T, K, idx, g, mode);
        if (kind == 0) continue;
        f.n_in++;
        if (kind == 1) continue;
        f.n_candidates++;
        const int d = fuse_hamming(qdesc, K.desc + 8 * (size_t)idx);
        if (d < f.best_dist) { f.best_dist = d; f.best_idx = idx; }
      }
    }
  return f;
}

}  // namespace osh
