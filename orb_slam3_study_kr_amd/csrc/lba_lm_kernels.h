// lba_lm_kernels.h -- local BA, one block per chunk of landmarks (lba_chunk.h): k_lin_lm, k_backsub, k_finalize, k_debug_hpl.
#pragma once
#include "lba_chunk.h"

namespace osh {
// --------------------------------------------------------------------------------------------
// k_lin_lm: the landmark side of the linearisation: residual, Huber weight, d err / d point of EVERY edge of the landmark
// (optimisable and fixed keyframes) ->
//   Hll_j = sum R^T Q R,  b_l(j) = sum R^T g   (summed per landmark in edge order by the landmark's own lane: fixed order)
//   chi2 partial and the largest Hll diagonal entry of the chunk (computeLambdaInit),
// then the landmark factor for the current lambda (landmark_factor(): setLambda + D->inverse(), block_solver.hpp:389,582-587).
// A window that is not linearising this round but whose lambda changed (first lambda of optimize(), rejected trial) only
// re-forms its factors from the stored Hll / b_l.
// --------------------------------------------------------------------------------------------
template <bool KB8, bool F32>
__global__ __launch_bounds__(kBlock) void k_lin_lm(BatchView bv) {
  extern __shared__ __attribute__((aligned(16))) double sh_lm[];   // LinLds (lba_view.h)
  const Chunk ch = bv.chunks[blockIdx.x];
  const WinDesc wd = bv.win[ch.win];   // by value: the fields stay in SGPRs across the kernel's stores
  const LmView st = lm_view(bv.lm, ch.win);
  if (!st.active || (!st.need_lin && !st.need_dl)) return;
  const int tid = threadIdx.x;
  const int nl = ch.lm1 - ch.lm0;
  const bool lambda_known = st.lambda >= 0.0;   // k_reset leaves -1 until k_control opened the first iteration
  if (!st.need_lin) {
    if (tid < nl) {
      const size_t gl = (size_t)wd.pt_off + ch.lm0 + tid;
      double hl[6], bl[3], dl[9];
#pragma unroll
      for (int k = 0; k < 6; ++k) hl[k] = bv.Hll[gl * 6 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) bl[k] = bv.bl[gl * 3 + k];
      dev::landmark_factor(hl, bl, st.lambda, dl);
#pragma unroll
      for (int k = 0; k < 9; ++k) bv.DL[gl * 9 + k] = dl[k];
    }
    return;
  }
  double* sh_c = sh_lm + LinLds::kPart;
  double* sh4 = sh_lm + LinLds::kRed;
  double* sh_X = sh_lm + LinLds::kX;
  double* sh_pose = sh_lm + LinLds::kPose;
  const double* poses = bv.pose_state[st.sel] + (size_t)wd.pose_off * 7;
  const double* pts = bv.pt_state[st.sel] + (size_t)wd.pt_off * 3;
  const double* cams = bv.pose_cam + (size_t)wd.pose_off * 5;
  const bool staged = (wd.P + wd.F) <= kLdsPoses;
  const int* lmo = bv.lm_off + wd.lmoff_off;
  const int e0 = lmo[ch.lm0], e1 = lmo[ch.lm1];
  int my_lo = 0, my_hi = 0;
  if (tid < nl) { my_lo = lmo[ch.lm0 + tid]; my_hi = lmo[ch.lm0 + tid + 1]; }
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  double chi_acc = 0.0;
  for (int base = e0; base < e1; base += kChunkMaxEdges) {
    LaneEdges le;
    load_lane_edges<F32>(bv, wd, base, e1, tid, le);
    if (base == e0) {
      stage_points(sh_X, pts, ch.lm0, nl, tid);
      if (staged) stage_poses(sh_pose, poses, cams, wd.P + wd.F, tid, kBlock);
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int pbase = base + p * kChunkEdges;
      if (pbase >= e1) break;     // uniform over the block
      const int e = pbase + tid;
      double hl[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) hl[k] = 0.0;
      if (e < e1) {
        double qt[7], cam[5], R[9], X[3], Xc[3], Q[6], g[3], rho0;
        fetch_pose(staged, sh_pose, poses, cams, le.ip[p], qt, cam, R);
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = sh_X[(le.il[p] - ch.lm0) * 3 + k];
        const double rec[4] = {le.ra[p].x, le.ra[p].y, le.rb[p].x, le.rb[p].y};
        win_edge_core<KB8>(wd, bv, (size_t)wd.edge_off + e, rec, qt, cam, R, X, Xc, Q, g, rho0);
        chi_acc += rho0;
        dev::core_landmark_side<KB8>(Q, g, R, hl);
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) sh_c[k * kChunkEdges + tid] = hl[k];
      __syncthreads();
      if (tid < nl) {
        const int lo = max(my_lo, pbase), hi = min(my_hi, pbase + kChunkEdges);
        for (int x = lo; x < hi; ++x) {
#pragma unroll
          for (int k = 0; k < 9; ++k) acc[k] += sh_c[k * kChunkEdges + x - pbase];
        }
      }
      __syncthreads();
    }
  }
  double dmax = 0.0;
  if (tid < nl) {
    const size_t gl = (size_t)wd.pt_off + ch.lm0 + tid;
#pragma unroll
    for (int k = 0; k < 6; ++k) bv.Hll[gl * 6 + k] = acc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) bv.bl[gl * 3 + k] = acc[6 + k];
    dmax = fmax(fabs(acc[0]), fmax(fabs(acc[3]), fabs(acc[5])));
    if (lambda_known) {
      double dl[9];
      dev::landmark_factor(acc, acc + 6, st.lambda, dl);
#pragma unroll
      for (int k = 0; k < 9; ++k) bv.DL[gl * 9 + k] = dl[k];
    }
  }
  const double chi = block_sum(chi_acc, sh4);
  dmax = block_max(dmax, sh4);
  if (tid == 0) { bv.chi_lin[blockIdx.x] = chi; bv.dmax_lin[blockIdx.x] = dmax; }
}

// --------------------------------------------------------------------------------------------
// k_backsub: x_l = (Hll + lambda I)^-1 (b_l - Hpl^T x_p) = F F^T (...), X_trial = X + x_l, landmark part of computeScale
// (block_solver.hpp:461-483, sparse_block_matrix_ccs.h:103-129).  Landmark-major (see above): lane per edge for the products
// -Hpl^T x_p = -R^T Q (D x_p) formed from the edge description (lba_math.h), lane per landmark for the ordered sum; the
// optimisable poses of the window and x_p sit in LDS.
// --------------------------------------------------------------------------------------------
template <bool KB8, bool F32>
__global__ __launch_bounds__(kBlock) void k_backsub(BatchView bv) {
  extern __shared__ __attribute__((aligned(16))) double sh_bs[];  // BacksubLds (lba_view.h)
  double* sh_c = sh_bs + BacksubLds::kPart;
  double* sh4 = sh_bs + BacksubLds::kRed;
  double* sh_X = sh_bs + BacksubLds::kX;
  double* sh_x = sh_bs + BacksubLds::kXp;
  const Chunk ch = bv.chunks[blockIdx.x];
  const WinDesc wd = bv.win[ch.win];   // by value: the fields stay in SGPRs across the kernel's stores
  const LmView st = lm_view(bv.lm, ch.win);
  if (!st.active) return;
  const int tid = threadIdx.x;
  const int n = wd.n;
  const double* poses = bv.pose_state[st.sel] + (size_t)wd.pose_off * 7;
  const double* cams = bv.pose_cam + (size_t)wd.pose_off * 5;
  const double* pts = bv.pt_state[st.sel] + (size_t)wd.pt_off * 3;
  const bool staged = backsub_stages(wd.P, wd.F);
  const double* xp = bv.xp + (size_t)wd.fpose_off * 6;
  const BacksubLds lds = BacksubLds::of(wd.P, wd.F, staged);
  double* sh_pose = sh_bs + lds.pose;
  const int* lmo = bv.lm_off + wd.lmoff_off;
  const int e0 = lmo[ch.lm0], e1 = lmo[ch.lm1];
  const int nl = ch.lm1 - ch.lm0;
  const double lambda = st.lambda;
  double acc[3] = {0, 0, 0};
  int my_lo = 0, my_hi = 0;
  double F[6], b3[3], Xcur[3];
#pragma unroll
  for (int k = 0; k < 6; ++k) F[k] = 0.0;
  b3[0] = b3[1] = b3[2] = 0.0; Xcur[0] = Xcur[1] = Xcur[2] = 0.0;
  if (tid < nl) {
    // the landmark's own data is requested with everything else
    const size_t gl = (size_t)wd.pt_off + ch.lm0 + tid;
    my_lo = lmo[ch.lm0 + tid]; my_hi = lmo[ch.lm0 + tid + 1];
#pragma unroll
    for (int k = 0; k < 6; ++k) F[k] = bv.DL[gl * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { b3[k] = bv.bl[gl * 3 + k]; Xcur[k] = pts[(size_t)(ch.lm0 + tid) * 3 + k]; }
  }
  for (int base = e0; base < e1; base += kChunkMaxEdges) {
    LaneEdges le;
    load_lane_edges<F32>(bv, wd, base, e1, tid, le);
    if (base == e0) {
      stage_points(sh_X, pts, ch.lm0, nl, tid);
      if (staged) {
        for (int k = tid; k < n; k += kBlock) sh_x[k] = xp[k];
        stage_poses(sh_pose, poses, cams, wd.P, tid, kBlock);
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int pbase = base + p * kChunkEdges;
      if (pbase >= e1) break;     // uniform over the block
      const int e = pbase + tid;
      double c[3] = {0, 0, 0};
      if (e < e1 && le.ip[p] < wd.P) {
        const int ip = le.ip[p];
        double qt[7], R[9], cam[5], X[3], Xc[3], Q[6], g[3], rho0, x6[6];
        fetch_pose(staged, sh_pose, poses, cams, ip, qt, cam, R);
#pragma unroll
        for (int k = 0; k < 6; ++k) x6[k] = staged ? sh_x[6 * ip + k] : xp[6 * ip + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = sh_X[(le.il[p] - ch.lm0) * 3 + k];
        const double rec[4] = {le.ra[p].x, le.ra[p].y, le.rb[p].x, le.rb[p].y};
        win_edge_core<KB8>(wd, bv, (size_t)wd.edge_off + e, rec, qt, cam, R, X, Xc, Q, g, rho0);
        dev::core_backsub<KB8>(Xc, Q, R, x6, c);
      }
      sh_c[tid] = c[0]; sh_c[kChunkEdges + tid] = c[1]; sh_c[2 * kChunkEdges + tid] = c[2];
      __syncthreads();
      if (tid < nl) {
        const int lo = max(my_lo, pbase), hi = min(my_hi, pbase + kChunkEdges);
        for (int x = lo; x < hi; ++x) {
          acc[0] += sh_c[x - pbase]; acc[1] += sh_c[kChunkEdges + x - pbase]; acc[2] += sh_c[2 * kChunkEdges + x - pbase];
        }
      }
      __syncthreads();
    }
  }
  double sc = 0.0;
  if (tid < nl) {
    const size_t gl = (size_t)wd.pt_off + ch.lm0 + tid;
    const double b0 = b3[0], b1 = b3[1], b2 = b3[2];
    const double c0 = b0 + acc[0], c1 = b1 + acc[1], c2 = b2 + acc[2];
    double xl[3];
    if (st.solve_ok) {
      // x_l = F (F^T c)
      const double t0 = F[0] * c0, t1 = F[1] * c0 + F[3] * c1, t2 = F[2] * c0 + F[4] * c1 + F[5] * c2;
      xl[0] = F[0] * t0 + F[1] * t1 + F[2] * t2;
      xl[1] = F[3] * t1 + F[4] * t2;
      xl[2] = F[5] * t2;
    } else {
      xl[0] = xl[1] = xl[2] = 0.0;
    }
    double* Xt = bv.pt_state[st.sel ^ 1] + gl * 3;
    Xt[0] = Xcur[0] + xl[0]; Xt[1] = Xcur[1] + xl[1]; Xt[2] = Xcur[2] + xl[2];
    sc = xl[0] * (lambda * xl[0] + b0) + xl[1] * (lambda * xl[1] + b1) + xl[2] * (lambda * xl[2] + b2);
  }
  sc = block_sum(sc, sh4);
  if (tid == 0) bv.scale_part[blockIdx.x] = sc;
  // ---- the trial residual of the chunk's edges (computeActiveErrors + activeRobustChi2 at the trial estimates, a pass of its own
  // until round 3): the chunk's trial landmarks are in this block's registers, the trial poses were written by k_solve before this
  // launch.  Same lane <-> edge mapping and the same sums as that pass: the chunk's chi2 is the same number.
  __syncthreads();
  if (tid < nl) {
    const double* Xt = bv.pt_state[st.sel ^ 1] + ((size_t)wd.pt_off + ch.lm0 + tid) * 3;   // (just written by this thread)
    sh_X[tid * 3] = Xt[0]; sh_X[tid * 3 + 1] = Xt[1]; sh_X[tid * 3 + 2] = Xt[2];
  }
  const double* poses_t = bv.pose_state[st.sel ^ 1] + (size_t)wd.pose_off * 7;
  const bool staged_t = lds.staged_t;
  double* sh_pose_t = sh_bs + lds.pose_t;
  if (staged_t) stage_poses(sh_pose_t, poses_t, cams, wd.P + wd.F, tid, kBlock);
  __syncthreads();
  double chi_acc = 0.0;
  for (int base = e0; base < e1; base += kChunkMaxEdges) {
    LaneEdges le;
    load_lane_edges<F32>(bv, wd, base, e1, tid, le);
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int e = base + p * kChunkEdges + tid;
      if (e < e1) {
        double qt[7], cam[5], R[9], X[3];
        fetch_pose(staged_t, sh_pose_t, poses_t, cams, le.ip[p], qt, cam, R);
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = sh_X[(le.il[p] - ch.lm0) * 3 + k];
        const double rec[4] = {le.ra[p].x, le.ra[p].y, le.rb[p].x, le.rb[p].y};
        double cl, cr;
        chi_acc += win_edge_rho<KB8>(wd, bv, (size_t)wd.edge_off + e, rec, qt, cam, R, X, cl, cr);
      }
    }
  }
  const double chi = block_sum(chi_acc, sh4);
  if (tid == 0) bv.chi_part[blockIdx.x] = chi;
}

// --------------------------------------------------------------------------------------------
// k_finalize: per-edge chi2 of the LAST evaluated errors (stale after a rejected final trial,
// levenberg.cpp:123-147) and isDepthPositive from the FINAL estimates (Optimizer.cc:1425), in the caller's edge order.
// A merged fisheye-rig edge reports to both of its caller edges.
// --------------------------------------------------------------------------------------------
// Landmark-major like its neighbours: the lane's edges of all passes are requested up front (load_lane_edges, the caller's edge
// index with them), the window's poses and the chunk's landmarks are parked in LDS behind one barrier, and the rest only computes.
// Two states can be needed: the one evaluated last (chi2) and the final one (depth sign).  They are the same buffer unless the
// window's last trial was rejected, and then only what the depth sign reads of the final state is staged beside the first:
// quaternion + translation and the landmarks.  chi2 through win_edge_rho and the sign through quat_rotate, as in k_finalize_plain
// below: the same bits (tests/test_gpu_lba_finalize.py).  Windows of more than kLdsPoses keyframes read their poses from global memory.
template <bool KB8, bool F32>
__global__ __launch_bounds__(kBlock) void k_finalize(BatchView bv) {
  extern __shared__ __attribute__((aligned(16))) double sh_fin[];   // FinLds (lba_view.h)
  const Chunk ch = bv.chunks[blockIdx.x];
  const WinDesc wd = bv.win[ch.win];   // by value: the fields stay in SGPRs across the kernel's stores
  const LmView st = lm_view(bv.lm, ch.win);
  const int tid = threadIdx.x;
  const int nl = ch.lm1 - ch.lm0;
  const int* lmo = bv.lm_off + wd.lmoff_off;
  const int e0 = lmo[ch.lm0], e1 = lmo[ch.lm1];
  const bool evaluated = st.iterations > 0;
  const int f = st.sel, s = evaluated ? st.last_eval_sel : f;
  const bool two = s != f;
  const int np = wd.P + wd.F;
  const bool staged = np <= kLdsPoses;
  double* sh_X = sh_fin + FinLds::kX;
  double* sh_Xf = two ? sh_fin + FinLds::kXf : sh_X;
  double* sh_pose = sh_fin + FinLds::kPose;
  double* sh_qf = sh_pose + np * kPoseRec;
  const double* poses = bv.pose_state[s] + (size_t)wd.pose_off * 7;
  const double* poses_f = bv.pose_state[f] + (size_t)wd.pose_off * 7;
  const double* cams = bv.pose_cam + (size_t)wd.pose_off * 5;
  const bool rig = KB8 && wd.kb8_on;
  for (int base = e0; base < e1; base += kChunkMaxEdges) {
    LaneEdges le;
    load_lane_edges<F32>(bv, wd, base, e1, tid, le);
    int eo[kPasses], ek[kPasses];
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const size_t ge = (size_t)wd.edge_off + min(base + p * kChunkEdges + tid, max(e1 - 1, 0));
      eo[p] = bv.e_orig[ge];
      ek[p] = rig ? bv.e_kind[ge] : kKindMono;
    }
    if (base == e0) {
      stage_points(sh_X, bv.pt_state[s] + (size_t)wd.pt_off * 3, ch.lm0, nl, tid);
      if (two) stage_points(sh_Xf, bv.pt_state[f] + (size_t)wd.pt_off * 3, ch.lm0, nl, tid);
      if (staged) {
        stage_poses(sh_pose, poses, cams, np, tid, kBlock);
        if (two) { for (int k = tid; k < 7 * np; k += kBlock) sh_qf[k] = poses_f[k]; }
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int e = base + p * kChunkEdges + tid;
      if (e >= e1) continue;
      const size_t ge = (size_t)wd.edge_off + e;
      const int ip = le.ip[p], li = le.il[p] - ch.lm0;
      double qt[7], cam[5], R[9], X[3];
      fetch_pose(staged, sh_pose, poses, cams, ip, qt, cam, R);
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] = sh_X[li * 3 + k];
      double chi_l = 0.0, chi_r = 0.0;
      if (evaluated) {
        const double rec[4] = {le.ra[p].x, le.ra[p].y, le.rb[p].x, le.rb[p].y};
        (void)win_edge_rho<KB8>(wd, bv, ge, rec, qt, cam, R, X, chi_l, chi_r);
      }
      if (two) {
#pragma unroll
        for (int k = 0; k < 7; ++k) qt[k] = staged ? sh_qf[ip * 7 + k] : poses_f[(size_t)ip * 7 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = sh_Xf[li * 3 + k];
      }
      double rot[3];
      dev::quat_rotate(qt, X, rot);
      const double Xl[3] = {rot[0] + qt[4], rot[1] + qt[5], rot[2] + qt[6]};
      const size_t go = (size_t)wd.out_off + eo[p];
      const int kind = ek[p];
      double zr = 0.0;
      if (KB8 && kind >= kKindBody) {   // isDepthPositive of the body edge: ((mTrl * T).map(X))(2) > 0
        double Xr[3];
        dev::quat_rotate(wd.trl, Xl, Xr);
        zr = Xr[2] + wd.trl[6];
      }
      if (kind == kKindBody) {
        bv.out_chi2[go] = chi_r;
        bv.out_depth[go] = zr > 0.0 ? 1 : 0;
      } else {
        bv.out_chi2[go] = chi_l;
        bv.out_depth[go] = (Xl[2] > 0.0) ? 1 : 0;
        if (kind == kKindBoth) {
          const size_t go2 = (size_t)wd.out_off + bv.e_orig2[ge];
          bv.out_chi2[go2] = chi_r;
          bv.out_depth[go2] = zr > 0.0 ? 1 : 0;
        }
      }
    }
  }
}

// The kernel above before it became landmark-major: each lane walks its edges one after the other and gathers the poses and landmarks
// of both states from global memory.  Kept as the control (OSH_LBA_FINALIZE_PLAIN at upload).
template <bool KB8>
__global__ __launch_bounds__(kBlock) void k_finalize_plain(BatchView bv) {
  const Chunk ch = bv.chunks[blockIdx.x];
  const WinDesc wd = bv.win[ch.win];   // by value: the fields stay in SGPRs across the kernel's stores
  const LmView st = lm_view(bv.lm, ch.win);
  const int* lmo = bv.lm_off + wd.lmoff_off;
  const int e0 = lmo[ch.lm0], e1 = lmo[ch.lm1];
  const bool evaluated = st.iterations > 0;
  for (int e = e0 + threadIdx.x; e < e1; e += kBlock) {
    const size_t ge = (size_t)wd.edge_off + e;
    const int ip = bv.e_pose[ge], il = bv.e_point[ge];
    double qt[7], cam[5], X[3], rec[4];
#pragma unroll
    for (int k = 0; k < 5; ++k) cam[k] = bv.pose_cam[((size_t)wd.pose_off + ip) * 5 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) rec[k] = bv.e_rec[ge * 4 + k];
    double chi_l = 0.0, chi_r = 0.0;
    if (evaluated) {
      const int s = st.last_eval_sel;
#pragma unroll
      for (int k = 0; k < 7; ++k) qt[k] = bv.pose_state[s][((size_t)wd.pose_off + ip) * 7 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] = bv.pt_state[s][((size_t)wd.pt_off + il) * 3 + k];
      double Re[9];
      dev::quat_to_R(qt, Re);
      (void)win_edge_rho<KB8>(wd, bv, ge, rec, qt, cam, Re, X, chi_l, chi_r);
    }
    const int f = st.sel;
#pragma unroll
    for (int k = 0; k < 7; ++k) qt[k] = bv.pose_state[f][((size_t)wd.pose_off + ip) * 7 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = bv.pt_state[f][((size_t)wd.pt_off + il) * 3 + k];
    double rot[3];
    dev::quat_rotate(qt, X, rot);
    const double Xl[3] = {rot[0] + qt[4], rot[1] + qt[5], rot[2] + qt[6]};
    const size_t go = (size_t)wd.out_off + bv.e_orig[ge];
    int kind = kKindMono;
    if (KB8 && wd.kb8_on) kind = bv.e_kind[ge];
    double zr = 0.0;
    if (KB8 && kind >= kKindBody) {   // isDepthPositive of the body edge: ((mTrl * T).map(X))(2) > 0
      double Xr[3];
      dev::quat_rotate(wd.trl, Xl, Xr);
      zr = Xr[2] + wd.trl[6];
    }
    if (kind == kKindBody) {
      bv.out_chi2[go] = chi_r;
      bv.out_depth[go] = zr > 0.0 ? 1 : 0;
    } else {
      bv.out_chi2[go] = chi_l;
      bv.out_depth[go] = (Xl[2] > 0.0) ? 1 : 0;
      if (kind == kKindBoth) {
        const size_t go2 = (size_t)wd.out_off + bv.e_orig2[ge];
        bv.out_chi2[go2] = chi_r;
        bv.out_depth[go2] = zr > 0.0 ? 1 : 0;
      }
    }
  }
}

// Debug / parity aid (osh_lba_linearize): the 6x3 blocks Hpl = D^T Q R of the optimisable-pose edges, which the
// optimisation itself never stores, in sorted edge order.
template <bool KB8>
__global__ __launch_bounds__(kBlock) void k_debug_hpl(BatchView bv, double* out) {
  const Chunk ch = bv.chunks[blockIdx.x];
  const WinDesc wd = bv.win[ch.win];
  const LmView st = lm_view(bv.lm, ch.win);
  const int* lmo = bv.lm_off + wd.lmoff_off;
  const int e0 = lmo[ch.lm0], e1 = lmo[ch.lm1];
  const double* poses = bv.pose_state[st.sel] + (size_t)wd.pose_off * 7;
  const double* cams = bv.pose_cam + (size_t)wd.pose_off * 5;
  const double* pts = bv.pt_state[st.sel] + (size_t)wd.pt_off * 3;
  for (int e = e0 + threadIdx.x; e < e1; e += kBlock) {
    const size_t ge = (size_t)wd.edge_off + e;
    const int ip = bv.e_pose[ge], il = bv.e_point[ge];
    double W[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) W[k] = 0.0;
    if (ip < wd.P) {
      double qt[7], cam[5], R[9], X[3], rec[4], Xc[3], Q[6], g[3], rho0;
      fetch_pose(false, nullptr, poses, cams, ip, qt, cam, R);
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] = pts[(size_t)il * 3 + k];
#pragma unroll
      for (int k = 0; k < 4; ++k) rec[k] = bv.e_rec[ge * 4 + k];
      win_edge_core<KB8>(wd, bv, ge, rec, qt, cam, R, X, Xc, Q, g, rho0);
      const double ident[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
      dev::core_WF<KB8>(Xc, Q, R, ident, W);
    }
#pragma unroll
    for (int k = 0; k < 18; ++k) out[ge * 18 + k] = W[k];
  }
}
}  // namespace osh
