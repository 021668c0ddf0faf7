// sim3opt_device.hip -- the relative-Sim3 refinement of a loop or merge candidate on MI355X (gfx950): HIP kernel + C-ABI driver.
//
// Replaces the solver part of ORB_SLAM3::Optimizer::OptimizeSim3 (src/Optimizer.cc:2118-2385): one VertexSim3Expmap
// (types_seven_dof_expmap.h:60-69, update[6] = 0 under _fix_scale), per matched pair an EdgeSim3ProjectXYZ (obs1 - cam1(S12 X2c))
// and an EdgeInverseSim3ProjectXYZ (obs2 - cam2(S12^-1 X1c)) (include/OptimizableTypes.h:175-215) whose Jacobians g2o takes by
// central differences (base_binary_edge.hpp:147-197, delta 1e-9), Huber kernels of delta (float)sqrt(th2) in round 1, and the
// Levenberg-Marquardt loop of optimization_algorithm_levenberg.cpp:99-169 (three-bad-iterations stop) with the dense 7x7 solve of
// LinearSolverDense.  The whole call -- optimize(5), the classification of the pairs by their last computed chi2, the early
// return under 10 inliers, optimize(nBad > 0 ? 10 : 5) without kernels and the final classification -- runs in ONE block per
// problem: thread per pair, fixed-order block reductions (bitwise reproducible, independent of the batch).  The budgets 5, 10 and 5
// are inputs (osh_sim3_problem.iterations, 0..OSH_SIM3_MAX_ITERATIONS each): a budget of 0 runs no iteration of its round, which
// lets tests/test_gpu_sim3_stages.py see one stage at a time in the ordinary outputs.
//
// Per linearisation the 14 perturbed states Sim3(+-delta e_d) * S12 (g2o's push / oplus / pop) and their inverses are formed once
// in LDS; g2o recomputes the same values for every edge, so the Jacobian bits are unchanged.
#include "common.h"
#include "lba_math.h"
#include "pgo_sim3.h"   // g2o::Sim3 restated; it also turns FMA contraction off for the rest of this file (central differences)
#include "block_kit.h"  // after pgo_sim3.h: the kit has no pragma of its own and is compiled without contraction here
#include "g2o_lm.h"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace osh {

constexpr int kST = 256;   // threads per problem block
constexpr int kSR = 36;    // reduced values per linearisation: upper(H) 28, b 7, robust chi2

struct Sim3Desc {
  int n, off, fix_scale;
  double S[8];
  double cam1[8], cam2[8];
  int kb8_1, kb8_2;
  float th2;
  double delta;   // Huber delta (double)(float)sqrt(th2)
  int iterations[3];   // optimize(N): round 1, round 2 when n_bad > 0, round 2 otherwise
};
struct Sim3Out {
  double S[8];
  double chi2_end[2];
  double H[28], b[7], chi2_lin;   // osh_sim3_linearize
  int iterations[2];
  int n_bad, n_in, round2;
};
struct Sim3View {
  const Sim3Desc* desc;
  Sim3Out* out;
  const double* X1c;   // [NP*3]
  const double* X2c;   // [NP*3]
  const double* obs1;  // [NP*2]
  const double* obs2;  // [NP*2]
  const double* info1; // [NP]
  const double* info2; // [NP]
  double* chi2_12;     // [NP] chi2 of the edges as last computed
  double* chi2_21;
  unsigned char* level;  // [NP] 1: round-1 outlier (edges removed), 2: final outlier, 0: inlier
};

// project(const Eigen::Vector3d&): Pinhole (src/CameraModels/Pinhole.cpp:35-41) or KannalaBrandt8 (lba_math.h, atan2f_rn)
template <bool KB8>
__device__ __forceinline__ void sim3_project(const double* cam, int kb8, const double* X, double& u, double& v) {
  if (KB8 && kb8) { dev::kb8_project(cam, cam + 4, X, u, v); return; }
  u = cam[0] * X[0] / X[2] + cam[2];
  v = cam[1] * X[1] / X[2] + cam[3];
}
// _error = obs - project(S.map(X))
template <bool KB8>
__device__ __forceinline__ void sim3_edge_error(const pgo::Sim3& S, const double* cam, int kb8, const double* X, const double* obs, double* e) {
  double P[3], u, v;
  pgo::sim3_map(S, X, P);
  sim3_project<KB8>(cam, kb8, P, u, v);
  e[0] = obs[0] - u;
  e[1] = obs[1] - v;
}
__device__ __forceinline__ double sim3_chi2(const double* e, double info) { return e[0] * (info * e[0]) + e[1] * (info * e[1]); }

__device__ __forceinline__ pgo::Sim3 sim3_lds(const double* p) { return pgo::sim3_load(p); }
// LDS of one block: current / trial estimate and its inverse, the 14 perturbed states and their inverses, the reductions
struct Sim3Shared {
  double S[2][8], Si[2][8];
  double P[14][8], Pi[14][8];
  double red[(kST / 64) * kSR];
  double sys[kSR];
  double x[7];
  double sh[kST / 64];
  int ok;
};

// the estimate `which` of sm and its inverse, by thread 0
__device__ __forceinline__ void sim3_set_state(Sim3Shared& sm, int which, const pgo::Sim3& S) {
  pgo::sim3_store(S, sm.S[which]);
  pgo::sim3_store(pgo::sim3_inverse(S), sm.Si[which]);
}

// computeActiveErrors + activeRobustChi2 at estimate `sel` over the active pairs (level 0); stores every active edge's chi2
template <bool KB8>
__device__ __forceinline__ double sim3_eval(const Sim3View& v, const Sim3Desc& d, Sim3Shared& sm, int sel, bool robust) {
  const pgo::Sim3 S = sim3_lds(sm.S[sel]), Si = sim3_lds(sm.Si[sel]);
  double acc = 0.0;
  for (int p = threadIdx.x; p < d.n; p += kST) {
    const size_t g = (size_t)d.off + p;
    if (v.level[g]) continue;
    double e12[2], e21[2];
    sim3_edge_error<KB8>(S, d.cam1, d.kb8_1, v.X2c + g * 3, v.obs1 + g * 2, e12);
    sim3_edge_error<KB8>(Si, d.cam2, d.kb8_2, v.X1c + g * 3, v.obs2 + g * 2, e21);
    const double c12 = sim3_chi2(e12, v.info1[g]), c21 = sim3_chi2(e21, v.info2[g]);
    v.chi2_12[g] = c12; v.chi2_21[g] = c21;
    if (robust) {
      double r0, r1;
      dev::huber(c12, d.delta, r0, r1); acc += r0;
      dev::huber(c21, d.delta, r0, r1); acc += r0;
    } else acc += c12 + c21;
  }
  return dev::block_sum_all<kST>(acc, sm.sh);
}

// one edge's contribution to H (upper, 28) and b (7): J = (e(+delta) - e(-delta)) / (2 delta) per column, H += J^T rho' Omega J,
// b += J^T (-rho' Omega e)
__device__ __forceinline__ void sim3_accumulate(const double (*J)[7], const double* e, double info, double r1, double* H, double* b) {
  const double ww = r1 * info;
  const double wr0 = -(info * e[0]) * r1, wr1 = -(info * e[1]) * r1;
  int m = 0;
#pragma unroll
  for (int a = 0; a < 7; ++a) {
    const double b0 = J[0][a] * ww, b1 = J[1][a] * ww;
#pragma unroll
    for (int c = a; c < 7; ++c) { H[m] += b0 * J[0][c] + b1 * J[1][c]; ++m; }
    b[a] += J[0][a] * wr0 + J[1][a] * wr1;
  }
}

// buildSystem at estimate `sel`: the perturbed states, every active pair's errors (stored as its chi2), Jacobians and weighted
// products, reduced into sm.sys (upper H 0..27, b 28..34, activeRobustChi2 35)
template <bool KB8>
__device__ __forceinline__ void sim3_linearize(const Sim3View& v, const Sim3Desc& d, Sim3Shared& sm, int sel, bool robust) {
  const int tid = threadIdx.x;
  if (tid < 14) {
    double u[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = k == (tid >> 1) ? ((tid & 1) ? -1e-9 : 1e-9) : 0.0;
    const pgo::Sim3 P = pgo::vertex_oplus(sim3_lds(sm.S[sel]), u, d.fix_scale != 0);
    pgo::sim3_store(P, sm.P[tid]);
    pgo::sim3_store(pgo::sim3_inverse(P), sm.Pi[tid]);
  }
  __syncthreads();
  const pgo::Sim3 S = sim3_lds(sm.S[sel]), Si = sim3_lds(sm.Si[sel]);
  const double scalar = 1.0 / (2 * 1e-9);
  double H[28], b[7], acc = 0.0;
#pragma unroll
  for (int k = 0; k < 28; ++k) H[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) b[k] = 0.0;
  for (int p = tid; p < d.n; p += kST) {
    const size_t g = (size_t)d.off + p;
    if (v.level[g]) continue;
    const double* X1 = v.X1c + g * 3;
    const double* X2 = v.X2c + g * 3;
    const double* o1 = v.obs1 + g * 2;
    const double* o2 = v.obs2 + g * 2;
    const double i1 = v.info1[g], i2 = v.info2[g];
    double e12[2], e21[2];
    sim3_edge_error<KB8>(S, d.cam1, d.kb8_1, X2, o1, e12);
    sim3_edge_error<KB8>(Si, d.cam2, d.kb8_2, X1, o2, e21);
    const double c12 = sim3_chi2(e12, i1), c21 = sim3_chi2(e21, i2);
    v.chi2_12[g] = c12; v.chi2_21[g] = c21;
    double r0_12 = c12, r1_12 = 1.0, r0_21 = c21, r1_21 = 1.0;
    if (robust) { dev::huber(c12, d.delta, r0_12, r1_12); dev::huber(c21, d.delta, r0_21, r1_21); }
    acc += r0_12 + r0_21;
    // one edge at a time (14 Jacobian entries live, not 28): e12 through the perturbed states, e21 through their inverses
    double J[2][7];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      // the perturbed states are read from LDS at their use: without this fence the 28 states (224 doubles) are hoisted out of
      // the pair loop into registers and spilled
      asm volatile("" ::: "memory");
      double ep[2], em[2];
      sim3_edge_error<KB8>(sim3_lds(sm.P[2 * c]), d.cam1, d.kb8_1, X2, o1, ep);
      sim3_edge_error<KB8>(sim3_lds(sm.P[2 * c + 1]), d.cam1, d.kb8_1, X2, o1, em);
      J[0][c] = scalar * (ep[0] - em[0]); J[1][c] = scalar * (ep[1] - em[1]);
    }
    sim3_accumulate(J, e12, i1, r1_12, H, b);
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      // the perturbed states are read from LDS at their use: without this fence the 28 states (224 doubles) are hoisted out of
      // the pair loop into registers and spilled
      asm volatile("" ::: "memory");
      double ep[2], em[2];
      sim3_edge_error<KB8>(sim3_lds(sm.Pi[2 * c]), d.cam2, d.kb8_2, X1, o2, ep);
      sim3_edge_error<KB8>(sim3_lds(sm.Pi[2 * c + 1]), d.cam2, d.kb8_2, X1, o2, em);
      J[0][c] = scalar * (ep[0] - em[0]); J[1][c] = scalar * (ep[1] - em[1]);
    }
    sim3_accumulate(J, e21, i2, r1_21, H, b);
  }
  double red[kSR];
#pragma unroll
  for (int k = 0; k < 28; ++k) red[k] = H[k];
#pragma unroll
  for (int k = 0; k < 7; ++k) red[28 + k] = b[k];
  red[35] = acc;
  dev::block_sum_n_to<kST, kSR>(red, sm.red, sm.sys);
  __syncthreads();
}

// initializeOptimization + optimize(iterations) from estimate `sel` over the pairs of level 0; returns the index of the final estimate
template <bool KB8>
__device__ int sim3_optimize(const Sim3View& v, const Sim3Desc& d, Sim3Shared& sm, int sel, int iterations, bool robust,
                             int& iters_out, double& chi_out) {
  const int tid = threadIdx.x;
  bool ok = true;
  double lambda = 0.0, ni = 2.0, currentChi = 0.0;
  int nBad = 0, cj = 0;
  for (int it = 0; it < iterations && ok; ++it) {
    sim3_linearize<KB8>(v, d, sm, sel, robust);
    currentChi = sm.sys[35];
    const double iniChi = currentChi;
    if (it == 0) {
      lambda = kLmTau * dev::upper_max_abs_diag<7>(sm.sys);   // computeLambdaInit
      ni = 2.0; nBad = 0;
    }
    double rho = 0.0;
    int qmax = 0;
    do {
      const int trs = sel ^ 1;
      if (tid == 0) {
        double x[7];
        // the dense 7x7 solve of LinearSolverDense: failure unless every pivot is positive
        const bool good = dev::ldlt_solve_upper<7>(sm.sys, sm.sys + 28, lambda, x);
        if (d.fix_scale) x[6] = 0;   // oplusImpl zeroes update[6] in the solver's own vector
        sim3_set_state(sm, trs, pgo::vertex_oplus(sim3_lds(sm.S[sel]), x, d.fix_scale != 0));
#pragma unroll
        for (int k = 0; k < 7; ++k) sm.x[k] = x[k];
        sm.ok = good ? 1 : 0;
      }
      __syncthreads();
      double tempChi = sim3_eval<KB8>(v, d, sm, trs, robust);
      if (!sm.ok) tempChi = DBL_MAX;
      double scale = 0.0;   // computeScale
#pragma unroll
      for (int k = 0; k < 7; ++k) scale += sm.x[k] * (lambda * sm.x[k] + sm.sys[28 + k]);
      const LmTrial trial = lm_judge_trial(lambda, ni, currentChi, tempChi, scale);
      rho = trial.rho;
      if (trial.accepted) { currentChi = tempChi; sel = trs; }
      qmax++;
      __syncthreads();
    } while (rho < 0 && qmax < kLmMaxTrials);
    ++cj;
    ok = lm_iteration_goes_on(nBad, iniChi, currentChi, qmax, rho);
  }
  iters_out = cj;
  chi_out = currentChi;
  return sel;
}

template <bool KB8>
__global__ __launch_bounds__(kST) void k_sim3_opt(Sim3View v) {
  __shared__ Sim3Shared sm;
  const Sim3Desc& d = v.desc[blockIdx.x];
  Sim3Out& out = v.out[blockIdx.x];
  const int tid = threadIdx.x;
  for (int p = tid; p < d.n; p += kST) { const size_t g = (size_t)d.off + p; v.level[g] = 0; v.chi2_12[g] = 0.0; v.chi2_21[g] = 0.0; }
  if (tid == 0) {
    sim3_set_state(sm, 0, pgo::sim3_load(d.S));
    for (int k = 0; k < 8; ++k) out.S[k] = d.S[k];
    out.iterations[0] = out.iterations[1] = 0;
    out.chi2_end[0] = out.chi2_end[1] = 0.0;
    out.n_bad = 0; out.n_in = 0; out.round2 = 0;
  }
  __syncthreads();
  if (d.n == 0) return;   // no pairs: nCorrespondences - nBad = 0 < 10, return 0
  const double th2 = (double)d.th2;   // a float threshold compared with the double chi2
  int sel = 0, n_bad = 0;
  // round 0: optimize(5) with Huber kernels over every pair; round 1: optimize(nBad > 0 ? 10 : 5) over the inliers without
  // kernels, from the round-0 estimate (one call site of the optimiser: the kernel is inlined once).  The budgets are
  // d.iterations, {5, 10, 5} from OptimizeSim3
  for (int round = 0; round < 2; ++round) {
    int iters = 0;
    double chi = 0.0;
    sel = sim3_optimize<KB8>(v, d, sm, sel, round == 0 ? d.iterations[0] : (n_bad > 0 ? d.iterations[1] : d.iterations[2]), round == 0, iters, chi);
    if (tid == 0) { out.iterations[round] = iters; out.chi2_end[round] = chi; }
    if (round == 0) {
      // classification by the chi2 each edge last computed (the last trial's, accepted or not)
      int bad = 0;
      for (int p = tid; p < d.n; p += kST) {
        const size_t g = (size_t)d.off + p;
        if (v.chi2_12[g] > th2 || v.chi2_21[g] > th2) { v.level[g] = 1; ++bad; }
      }
      n_bad = (int)dev::block_sum_all<kST>((double)bad, sm.sh);
      if (tid == 0) out.n_bad = n_bad;
      if (d.n - n_bad < 10) return;   // g2oS12 and mAcumHessian untouched, return 0
    }
  }
  // computeError at the final estimate and the final classification
  const pgo::Sim3 S = sim3_lds(sm.S[sel]), Si = sim3_lds(sm.Si[sel]);
  int in = 0;
  for (int p = tid; p < d.n; p += kST) {
    const size_t g = (size_t)d.off + p;
    if (v.level[g]) continue;
    double e12[2], e21[2];
    sim3_edge_error<KB8>(S, d.cam1, d.kb8_1, v.X2c + g * 3, v.obs1 + g * 2, e12);
    sim3_edge_error<KB8>(Si, d.cam2, d.kb8_2, v.X1c + g * 3, v.obs2 + g * 2, e21);
    const double c12 = sim3_chi2(e12, v.info1[g]), c21 = sim3_chi2(e21, v.info2[g]);
    v.chi2_12[g] = c12; v.chi2_21[g] = c21;
    if (c12 > th2 || c21 > th2) v.level[g] = 2; else ++in;
  }
  const int n_in = (int)dev::block_sum_all<kST>((double)in, sm.sh);
  if (tid == 0) {
    out.round2 = 1; out.n_in = n_in;
    for (int k = 0; k < 8; ++k) out.S[k] = sm.S[sel][k];
  }
}

// osh_sim3_linearize: the first buildSystem of round 0 (robust kernels) at the initial estimate
template <bool KB8>
__global__ __launch_bounds__(kST) void k_sim3_lin(Sim3View v) {
  __shared__ Sim3Shared sm;
  const Sim3Desc& d = v.desc[blockIdx.x];
  Sim3Out& out = v.out[blockIdx.x];
  const int tid = threadIdx.x;
  for (int p = tid; p < d.n; p += kST) v.level[(size_t)d.off + p] = 0;
  if (tid == 0) sim3_set_state(sm, 0, pgo::sim3_load(d.S));
  __syncthreads();
  if (d.n > 0) sim3_linearize<KB8>(v, d, sm, 0, true);
  if (tid < 28) out.H[tid] = d.n > 0 ? sm.sys[tid] : 0.0;
  else if (tid < 35) out.b[tid - 28] = d.n > 0 ? sm.sys[tid] : 0.0;
  else if (tid == 35) out.chi2_lin = d.n > 0 ? sm.sys[35] : 0.0;
}

// validate, stage, launch, copy back: the shared body of osh_sim3_optimize (lin_only 0) and osh_sim3_linearize (lin_only 1)
static int sim3_run(osh_lba_ctx* ctx, int n, const osh_sim3_problem* pr, int lin_only, std::vector<Sim3Out>& outs,
                    std::vector<unsigned char>& level, std::vector<double>& c12, std::vector<double>& c21, std::vector<int>& offs) {
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(lba_stream(ctx, &device, &s));
  std::vector<Sim3Desc> h_desc(n);
  size_t NP = 0;
  bool any_kb8 = false;
  offs.assign(n, 0);
  for (int f = 0; f < n; ++f) {
    const osh_sim3_problem& p = pr[f];
    if (p.n_pairs < 0 || (p.n_pairs > 0 && (!p.X1c || !p.X2c || !p.obs1 || !p.obs2 || !p.info1 || !p.info2))) {
      set_error("problem %d: negative size or NULL array", f); return OSH_ERR_INVALID;
    }
    if (!(p.th2 > 0.0f) || !std::isfinite(p.th2)) { set_error("problem %d: th2 must be positive and finite", f); return OSH_ERR_INVALID; }
    if (!(p.S12[7] > 0.0) || !std::isfinite(p.S12[7])) { set_error("problem %d: the scale of S12 must be positive and finite", f); return OSH_ERR_INVALID; }
    if ((p.kb8_1 != 0 && p.kb8_1 != 1) || (p.kb8_2 != 0 && p.kb8_2 != 1)) { set_error("problem %d: camera model out of range", f); return OSH_ERR_INVALID; }
    for (int k = 0; k < 3; ++k)
      if (p.iterations[k] < 0 || p.iterations[k] > OSH_SIM3_MAX_ITERATIONS) {
        set_error("problem %d: iterations[%d] = %d outside 0..%d", f, k, p.iterations[k], OSH_SIM3_MAX_ITERATIONS); return OSH_ERR_INVALID;
      }
    Sim3Desc& d = h_desc[f];
    std::memset(&d, 0, sizeof(d));
    d.n = p.n_pairs; d.off = (int)NP; d.fix_scale = p.fix_scale ? 1 : 0;
    for (int k = 0; k < 8; ++k) { d.S[k] = p.S12[k]; d.cam1[k] = p.cam1[k]; d.cam2[k] = p.cam2[k]; }
    d.kb8_1 = p.kb8_1; d.kb8_2 = p.kb8_2;
    for (int k = 0; k < 3; ++k) d.iterations[k] = p.iterations[k];
    any_kb8 = any_kb8 || p.kb8_1 || p.kb8_2;
    d.th2 = p.th2;
    d.delta = (double)std::sqrt(p.th2);   // const float deltaHuber = sqrt(th2) (src/Optimizer.cc:2165)
    offs[f] = (int)NP;
    NP += (size_t)p.n_pairs;
  }
  if (NP > 0x7fffff00u) { set_error("batch too large for 32-bit offsets"); return OSH_ERR_UNSUPPORTED; }
  Layout in, out;
  const auto i_desc = in.take<Sim3Desc>(n);
  const auto i_X1 = in.take<double>(NP * 3), i_X2 = in.take<double>(NP * 3), i_o1 = in.take<double>(NP * 2), i_o2 = in.take<double>(NP * 2),
             i_i1 = in.take<double>(NP), i_i2 = in.take<double>(NP);
  const auto o_out = out.take<Sim3Out>(n);
  const auto o_c12 = out.take<double>(NP), o_c21 = out.take<double>(NP);
  const auto o_level = out.take<unsigned char>(NP);
  StagedCall* B = attachment<StagedCall>(ctx, kAttachSim3);
  if (!B) return OSH_ERR_INVALID;
  OSH_TRY(B->reserve(in, out));
  char* const hs = B->host_in();
  std::memcpy(i_desc.in(hs), h_desc.data(), n * sizeof(Sim3Desc));
  for (int f = 0; f < n; ++f) {
    const osh_sim3_problem& p = pr[f];
    const size_t o = (size_t)offs[f], np = (size_t)p.n_pairs;
    if (np == 0) continue;
    std::memcpy(i_X1.in(hs) + o * 3, p.X1c, np * 24);
    std::memcpy(i_X2.in(hs) + o * 3, p.X2c, np * 24);
    std::memcpy(i_o1.in(hs) + o * 2, p.obs1, np * 16);
    std::memcpy(i_o2.in(hs) + o * 2, p.obs2, np * 16);
    std::memcpy(i_i1.in(hs) + o, p.info1, np * 8);
    std::memcpy(i_i2.in(hs) + o, p.info2, np * 8);
  }
  OSH_TRY(B->upload(s));
  char* const din = B->dev_in();
  char* const dout = B->dev_out();
  Sim3View v;
  v.desc = i_desc.in(din); v.out = o_out.in(dout);
  v.X1c = i_X1.in(din); v.X2c = i_X2.in(din); v.obs1 = i_o1.in(din); v.obs2 = i_o2.in(din); v.info1 = i_i1.in(din); v.info2 = i_i2.in(din);
  v.chi2_12 = o_c12.in(dout); v.chi2_21 = o_c21.in(dout); v.level = o_level.in(dout);
  if (lin_only) {
    if (any_kb8) hipLaunchKernelGGL(k_sim3_lin<true>, dim3((unsigned)n), dim3(kST), 0, s, v);
    else hipLaunchKernelGGL(k_sim3_lin<false>, dim3((unsigned)n), dim3(kST), 0, s, v);
  } else {
    if (any_kb8) hipLaunchKernelGGL(k_sim3_opt<true>, dim3((unsigned)n), dim3(kST), 0, s, v);
    else hipLaunchKernelGGL(k_sim3_opt<false>, dim3((unsigned)n), dim3(kST), 0, s, v);
  }
  OSH_TRY(launch_check(lin_only ? "k_sim3_lin" : "k_sim3_opt"));
  OSH_TRY(B->download(s));
  char* const hr = B->host_out();
  outs.assign(o_out.in(hr), o_out.in(hr) + n);
  level.assign(o_level.in(hr), o_level.in(hr) + NP);
  c12.assign(o_c12.in(hr), o_c12.in(hr) + NP);
  c21.assign(o_c21.in(hr), o_c21.in(hr) + NP);
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_sim3_optimize(osh_lba_ctx* ctx, int32_t n, const osh_sim3_problem* pr, osh_sim3_result* res) {
  if (!ctx || n <= 0 || !pr || !res) { set_error("osh_sim3_optimize: bad arguments"); return OSH_ERR_INVALID; }
  std::vector<Sim3Out> outs;
  std::vector<unsigned char> level;
  std::vector<double> c12, c21;
  std::vector<int> offs;
  OSH_TRY(sim3_run(ctx, n, pr, 0, outs, level, c12, c21, offs));
  for (int f = 0; f < n; ++f) {
    osh_sim3_result& r = res[f];
    const Sim3Out& o = outs[f];
    for (int k = 0; k < 8; ++k) r.S12[k] = o.S[k];
    r.n_bad = o.n_bad; r.n_in = o.n_in; r.round2 = o.round2;
    for (int k = 0; k < 2; ++k) { r.iterations[k] = o.iterations[k]; r.chi2_end[k] = o.chi2_end[k]; }
    r.status = OSH_OK;
    const size_t off = (size_t)offs[f];
    for (int p = 0; p < pr[f].n_pairs; ++p) {
      const unsigned char lv = level[off + p];
      if (r.outlier1) r.outlier1[p] = lv == 1 ? 1 : 0;
      if (r.outlier) r.outlier[p] = lv != 0 ? 1 : 0;
      if (r.chi2_12) r.chi2_12[p] = c12[off + p];
      if (r.chi2_21) r.chi2_21[p] = c21[off + p];
    }
  }
  return OSH_OK;
}

extern "C" int osh_sim3_linearize(osh_lba_ctx* ctx, const osh_sim3_problem* pr, double* H, double* b, double* chi2) {
  if (!ctx || !pr || !H || !b || !chi2) { set_error("osh_sim3_linearize: bad arguments"); return OSH_ERR_INVALID; }
  std::vector<Sim3Out> outs;
  std::vector<unsigned char> level;
  std::vector<double> c12, c21;
  std::vector<int> offs;
  OSH_TRY(sim3_run(ctx, 1, pr, 1, outs, level, c12, c21, offs));
  const Sim3Out& o = outs[0];
  int m = 0;
  for (int a = 0; a < 7; ++a)
    for (int c = a; c < 7; ++c) { H[a * 7 + c] = o.H[m]; H[c * 7 + a] = o.H[m]; ++m; }
  for (int k = 0; k < 7; ++k) b[k] = o.b[k];
  *chi2 = o.chi2_lin;
  return OSH_OK;
}
