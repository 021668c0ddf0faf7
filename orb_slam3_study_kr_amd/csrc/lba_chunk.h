// lba_chunk.h -- device only, shared by the landmark-major kernels and the Schur items: the edge description through the window's
// camera model, the staged pose record, the lane's edges of a chunk.  DESIGN.md section 25.
#pragma once
#include "lba_view.h"

namespace osh {
// Edge description (lba_math.h) of sorted edge `ge` through the window's camera model.  KB8 is a compile-time switch: the
// pinhole instantiations of the kernels (every batch without a fisheye window) carry no KannalaBrandt8 code or registers.
// chi_l / chi_r are only meaningful for KB8 windows (per-edge chi2 of a merged rig edge).
template <bool KB8>
__device__ __forceinline__ void win_edge_core(const WinDesc& wd, const BatchView& bv, size_t ge, const double* rec, const double* qt,
                                              const double* cam, const double* R, const double* X, double* Xc, double* Q, double* g, double& rho0) {
  if (KB8 && wd.kb8_on) {
    double cl, cr;
    double rec2[4] = {0.0, 0.0, 0.0, 0.0};
    const int kind = bv.e_kind[ge];
    if (kind == kKindBoth) {
#pragma unroll
      for (int k = 0; k < 4; ++k) rec2[k] = bv.e_rec2[ge * 4 + k];
    }
    dev::edge_core_kb8(kind, qt, cam, wd.kb8, wd.cam2, wd.trl, X, rec, rec2, wd.huber_mono, Xc, Q, g, rho0, cl, cr);
    return;
  }
  dev::edge_core_pinhole(R, qt + 4, cam, X, rec, wd.huber_mono, wd.huber_stereo, Xc, Q, g, rho0);
}

// Robustified chi2 of sorted edge `ge` (the trial residual needs nothing else); chi_l / chi_r as above.
template <bool KB8>
__device__ __forceinline__ double win_edge_rho(const WinDesc& wd, const BatchView& bv, size_t ge, const double* rec, const double* qt,
                                               const double* cam, const double* R, const double* X, double& chi_l, double& chi_r) {
  if (KB8 && wd.kb8_on) {
    double Xc[3], Q[6], g[3], rho0;
    double rec2[4] = {0.0, 0.0, 0.0, 0.0};
    const int kind = bv.e_kind[ge];
    if (kind == kKindBoth) {
#pragma unroll
      for (int k = 0; k < 4; ++k) rec2[k] = bv.e_rec2[ge * 4 + k];
    }
    dev::edge_core_kb8(kind, qt, cam, wd.kb8, wd.cam2, wd.trl, X, rec, rec2, wd.huber_mono, Xc, Q, g, rho0, chi_l, chi_r);
    return rho0;
  }
  const bool stereo = rec[3] > 0.0;
  double r[3], Xc[3], rho0, rho1, iz;
  chi_l = dev::edge_residual_pinhole(R, qt + 4, cam, X, rec, r, Xc, iz);   // the same expressions as win_edge_core: chi2 of a state is one number
  chi_r = 0.0;
  dev::huber_fast(chi_l, stereo ? wd.huber_stereo : wd.huber_mono, rho0, rho1);
  return rho0;
}

// Stages the window's poses (quaternion + translation, camera, rotation matrix) in LDS for a landmark-major block.
__device__ __forceinline__ void stage_poses(double* sh_pose, const double* poses, const double* cams, int n_poses, int tid, int nthreads) {
  for (int i = tid; i < n_poses; i += nthreads) {
    double qt[7], R[9];
#pragma unroll
    for (int k = 0; k < 7; ++k) qt[k] = poses[(size_t)i * 7 + k];
    dev::quat_to_R(qt, R);
#pragma unroll
    for (int k = 0; k < 7; ++k) sh_pose[i * kPoseRec + k] = qt[k];
#pragma unroll
    for (int k = 0; k < 5; ++k) sh_pose[i * kPoseRec + 7 + k] = cams[(size_t)i * 5 + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) sh_pose[i * kPoseRec + 12 + k] = R[k];
  }
}
__device__ __forceinline__ void fetch_pose(bool staged, const double* sh_pose, const double* poses, const double* cams, int ip,
                                           double* qt, double* cam, double* R) {
  if (staged) {
#pragma unroll
    for (int k = 0; k < 7; ++k) qt[k] = sh_pose[ip * kPoseRec + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) cam[k] = sh_pose[ip * kPoseRec + 7 + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = sh_pose[ip * kPoseRec + 12 + k];
  } else {
#pragma unroll
    for (int k = 0; k < 7; ++k) qt[k] = poses[(size_t)ip * 7 + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) cam[k] = cams[(size_t)ip * 5 + k];
    dev::quat_to_R(qt, R);
  }
}

// --------------------------------------------------------------------------------------------
// Landmark-major kernels (k_lin_lm, k_backsub): one block per chunk of consecutive landmarks (<= 1024 edges,
// <= 256 landmarks), lane per edge in kPasses passes of 256.  The block first requests everything it will touch -- the
// lane's edges of all passes (pose index, landmark index, observation record), the chunk's landmarks (coalesced) and the
// window's poses -- parks the shared part in LDS behind ONE barrier and then only computes: one memory round trip per block
// instead of two per pass.  (A wavefront-granular variant -- chunks of 64 edges, no block barriers, per-landmark sums as
// parallel (landmark, component) tasks -- was measured 2x SLOWER: the per-chunk reduction and the cold start of every
// short-lived wavefront cost more than the four barriers of a 1024-edge block.)
// --------------------------------------------------------------------------------------------

struct LaneEdges { int ip[kPasses], il[kPasses]; double2 ra[kPasses], rb[kPasses]; };

// edges base + p * 256 + tid, p = 0..kPasses-1, clamped to the last edge of the chunk (validity is applied at use)
// F32: the records are read as the float32 values they were uploaded as (exact: the packer checked) -- 16 bytes an edge instead of
// 32 in the bandwidth-bound landmark-major kernels.  A compile-time choice: a run-time test in this loop splits the block of
// loads the kernels issue up front (measured: k_lin_lm 0.68 -> 1.09 ms with the branch, 0.56 ms without).
template <bool F32>
__device__ __forceinline__ void load_lane_edges(const BatchView& bv, const WinDesc& wd, int base, int e1, int tid, LaneEdges& le) {
  const int last = max(e1 - 1, 0);
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const size_t ge = (size_t)wd.edge_off + min(base + p * kChunkEdges + tid, last);
    le.ip[p] = bv.e_pose[ge];
    le.il[p] = bv.e_point[ge];
    if (F32) {
      const float4 r = bv.e_rec32[ge];
      le.ra[p] = make_double2((double)r.x, (double)r.y); le.rb[p] = make_double2((double)r.z, (double)r.w);
    } else {
      const double2* r = reinterpret_cast<const double2*>(bv.e_rec + ge * 4);
      le.ra[p] = r[0]; le.rb[p] = r[1];
    }
  }
}

// the chunk's landmarks -> LDS [nl][3] (coalesced: consecutive landmarks are consecutive in memory)
__device__ __forceinline__ void stage_points(double* sh_X, const double* pts, int lm0, int nl, int tid) {
  for (int k = tid; k < 3 * nl; k += kBlock) sh_X[k] = pts[(size_t)lm0 * 3 + k];
}
}  // namespace osh
