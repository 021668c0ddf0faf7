// pgo4_device.hip -- the 4-DoF pose graph of Optimizer::OptimizeEssentialGraph4DoF on the device (include/orbslam3_hip.h,
// osh_pgo4_*).  One VertexPose4DoF per keyframe, Edge4DoF with a diagonal information, g2o's central-difference Jacobians,
// Levenberg-Marquardt as optimization_algorithm_levenberg.cpp:99-169 runs it, lambda_0 from computeLambdaInit (:171-184)
// unless the caller gives one.  The controller stays on the host, as for the Sim3 graph.
//
// A vertex is its full ImuCamPose state (pgo4_se3.h): g2o evaluates every Jacobian column and every trial on a pushed copy
// of the vertex, so the update count `its` and the yaw accumulator DR travel with the pose, and a perturbed evaluation at
// its == 4 runs the normalisation of DR exactly as the reference does.
//
// Kernels, in the order of one trial:
//   k_pgo4_lin       thread per edge: error, chi2 = e^T Omega e and the two 6x4 numeric Jacobians (delta 1e-9) at linearisation
//   k_pgo_assemble   block per 4x4 block of H: sums its edges in edge order (CSR built at upload, no atomics); b = -J^T Omega e
//                    (pgo_env.h, with the diagonal Omega)
//   k_pgo_maxdiag    once, when lambda_0 is g2o's: max |diag H| over the free vertices (pgo_env.h)
//   k_pgo_fill       H + lambda I into the envelope tiles (8 vertices per 32-wide tile), b into the right-hand side (pgo_env.h)
//   k_env_*          the Sim3 graph's envelope LDL^T, unchanged (pgo_env.h)
//   k_pgo4_step      UpdateW of every free vertex into the candidate state
//   k_pgo4_lin (errors only) and k_pgo_reduce: chi2 and computeScale in a fixed order
//
// This file holds the 4-DoF vertex and edge (Pgo4Graph): k_pgo4_lin, k_pgo4_step, the validation, the packing of the vertex
// states and the write-back.  The trial sequence and the LM loop are the Sim3 graph's (pgo_env.h).
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "common.h"
#include "pgo4_se3.h"
#include "pgo_env.h"

namespace osh {
namespace {

using pgo4::kConstDoubles;
using pgo4::kStateDoubles;

struct Info6 {
  double w[6];
};

struct Pgo4View {
  const double* st;               // [n][34] vertex states the edges are evaluated at
  const double* cst;              // [n][21] Rwb0 Rcb tcb
  const int* eij;                 // [E][2]
  const double* meas;             // [E][12] dR dt
  const int* sys;                 // [n] index of the free vertex, -1 when fixed
  double* J;                      // [E][2][24]  d e_r / d x_c, row-major 6x4
  double* err;                    // [E][6]
  double* chi;                    // [E]
  Info6 info;
  int E;
};

__global__ __launch_bounds__(64) void k_pgo4_lin(Pgo4View v, int linearize) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= v.E) return;
  using namespace pgo4;
  const int vi = v.eij[2 * e], vj = v.eij[2 * e + 1];
  const double* dR = v.meas + 12 * (size_t)e;
  const double* dt = dR + 9;
  const State Si = state_load(v.st + kStateDoubles * (size_t)vi), Sj = state_load(v.st + kStateDoubles * (size_t)vj);
  double e0[6];
  edge_error(dR, dt, Si.Rcw, Si.tcw, Sj.Rcw, Sj.tcw, e0);
  double c2 = 0;
  for (int k = 0; k < 6; ++k) { v.err[6 * (size_t)e + k] = e0[k]; c2 += e0[k] * (v.info.w[k] * e0[k]); }
  v.chi[e] = c2;
  if (!linearize) return;
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  for (int side = 0; side < 2; ++side) {
    const int vx = side ? vj : vi;
    if (v.sys[vx] < 0) continue;
    const Const C = const_load(v.cst + kConstDoubles * (size_t)vx);
    const State& X = side ? Sj : Si;
    double* Jo = v.J + ((size_t)e * 2 + side) * 24;
    for (int d = 0; d < 4; ++d) {
      double add[4] = {0, 0, 0, 0}, ep[6], em[6];
      add[d] = delta;
      State Xp = X;
      update_w(Xp, C, add);
      if (side) edge_error(dR, dt, Si.Rcw, Si.tcw, Xp.Rcw, Xp.tcw, ep); else edge_error(dR, dt, Xp.Rcw, Xp.tcw, Sj.Rcw, Sj.tcw, ep);
      add[d] = -delta;
      State Xm = X;
      update_w(Xm, C, add);
      if (side) edge_error(dR, dt, Si.Rcw, Si.tcw, Xm.Rcw, Xm.tcw, em); else edge_error(dR, dt, Xm.Rcw, Xm.tcw, Sj.Rcw, Sj.tcw, em);
      for (int r = 0; r < 6; ++r) { double bak = ep[r]; bak -= em[r]; Jo[r * 4 + d] = scalar * bak; }
    }
  }
}

struct Asm4View : AsmArrays {
  Info6 info;
  int nblk;
};

__global__ __launch_bounds__(64) void k_pgo4_step(const double* st, double* st_new, const double* cst, const int* sys, const double* x,
                                                  const int* fail, int n) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n) return;
  const int a = sys[v];
  if (a < 0 || *fail) {
    for (int k = 0; k < kStateDoubles; ++k) st_new[kStateDoubles * (size_t)v + k] = st[kStateDoubles * (size_t)v + k];
    return;
  }
  pgo4::State s = pgo4::state_load(st + kStateDoubles * (size_t)v);
  pgo4::update_w(s, pgo4::const_load(cst + kConstDoubles * (size_t)v), x + 4 * (size_t)a);
  pgo4::state_store(s, st_new + kStateDoubles * (size_t)v);
}

int validate4(const osh_pgo4_problem* p) {
  if (!p || p->n_vertices <= 0 || p->n_edges < 0 || !p->Rwb || !p->twb || !p->Rcw || !p->tcw || !p->Rcb || !p->tcb || !p->fixed ||
      (p->n_edges > 0 && (!p->edge_ij || !p->dR || !p->dt))) {
    set_error("osh_pgo4: bad problem (sizes or NULL arrays)");
    return OSH_ERR_INVALID;
  }
  if (p->solve_mode != OSH_PGO_SOLVE_ENVELOPE && p->solve_mode != OSH_PGO_SOLVE_DENSE) { set_error("osh_pgo4: unknown solve_mode"); return OSH_ERR_INVALID; }
  if (!(p->lambda_init >= 0) || !std::isfinite(p->lambda_init)) { set_error("osh_pgo4: lambda_init must be >= 0 and finite"); return OSH_ERR_INVALID; }
  for (int k = 0; k < 6; ++k)
    if (!(p->info_diag[k] >= 0) || !std::isfinite(p->info_diag[k])) { set_error("osh_pgo4: info_diag must be >= 0 and finite"); return OSH_ERR_INVALID; }
  if (p->iterations < 0) { set_error("osh_pgo4: negative iterations"); return OSH_ERR_INVALID; }
  return OSH_OK;
}

struct Pgo4Graph {
  static constexpr int D = 4, M = 6, kState = kStateDoubles, kMeas = 12, kAux = kConstDoubles;
  static constexpr bool kDiagInfo = true;
  using Aux = double;   // Rwb0 Rcb tcb
  static constexpr const char* kTag = "osh_pgo4";
  Info6 info;

  template <class R> Asm4View asm_view(const R& r) const { return Asm4View{r.asm_arrays(), info, r.P.nblk}; }
  template <class R> int lin(const R& r, int cur, int linearize) const {
    Pgo4View v;
    v.st = r.d_x[cur]; v.cst = r.d_aux; v.eij = r.d_eij; v.meas = r.d_meas; v.sys = r.d_sys; v.J = r.d_J; v.err = r.d_err;
    v.chi = r.d_chi; v.info = info; v.E = r.P.E;
    if (r.P.E > 0) hipLaunchKernelGGL(k_pgo4_lin, dim3((unsigned)((r.P.E + 63) / 64)), dim3(64), 0, r.s, v, linearize);
    return launch_check("k_pgo4_lin");
  }
  template <class R> int step(const R& r, int cur) const {
    hipLaunchKernelGGL(k_pgo4_step, dim3((unsigned)((r.P.n + 63) / 64)), dim3(64), 0, r.s, r.d_x[cur], r.d_x[1 - cur], r.d_aux, r.d_sys,
                       r.d_w, r.d_fail, r.P.n);
    return launch_check("k_pgo4_step");
  }
};

using Run4 = PgoRun<Pgo4Graph>;

// validation and the plan: no device work
int check4(Run4& R, const osh_pgo4_problem* p) {
  OSH_TRY(validate4(p));
  for (int k = 0; k < 6; ++k) R.graph.info.w[k] = p->info_diag[k];
  return R.plan(PlanInput{p->n_vertices, p->n_edges, p->solve_mode, p->fixed, p->edge_ij});
}

// the initial vertex states (DR = I, its = 0, the raw camera pose) and the constants, packed on the host
int upload4(Run4& R, const osh_pgo4_problem* p) {
  const size_t n = R.P.n;
  std::vector<double> st(n * kStateDoubles), cst(n * kConstDoubles), meas((size_t)R.P.E * 12);
  for (size_t v = 0; v < n; ++v) {
    double* o = st.data() + v * kStateDoubles;
    for (int k = 0; k < 9; ++k) o[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int k = 0; k < 9; ++k) o[9 + k] = p->Rwb[9 * v + k];
    for (int k = 0; k < 3; ++k) o[18 + k] = p->twb[3 * v + k];
    for (int k = 0; k < 9; ++k) o[21 + k] = p->Rcw[9 * v + k];
    for (int k = 0; k < 3; ++k) o[30 + k] = p->tcw[3 * v + k];
    o[33] = 0.0;
    double* c = cst.data() + v * kConstDoubles;
    for (int k = 0; k < 9; ++k) c[k] = p->Rwb[9 * v + k];
    for (int k = 0; k < 9; ++k) c[9 + k] = p->Rcb[9 * v + k];
    for (int k = 0; k < 3; ++k) c[18 + k] = p->tcb[3 * v + k];
  }
  for (int e = 0; e < R.P.E; ++e) {
    for (int k = 0; k < 9; ++k) meas[12 * (size_t)e + k] = p->dR[9 * (size_t)e + k];
    for (int k = 0; k < 3; ++k) meas[12 * (size_t)e + 9 + k] = p->dt[3 * (size_t)e + k];
  }
  OSH_TRY(R.upload(st.data(), meas.data(), p->edge_ij, cst.data()));
  // the host vectors go out of scope: wait for the copies
  OSH_HIP(hipStreamSynchronize(R.s));
  return OSH_OK;
}

}  // namespace
}  // namespace osh

using namespace osh;

extern "C" int osh_pgo4_solve(osh_lba_ctx* ctx, const osh_pgo4_problem* p, osh_pgo4_result* res) {
  if (!ctx || !res || !res->Rcw || !res->tcw) { set_error("osh_pgo4_solve: bad arguments"); return OSH_ERR_INVALID; }
  Run4 R(ctx);
  OSH_TRY(check4(R, p));   // refusals leave the result untouched
  res->status = OSH_ERR_DEVICE;
  OSH_TRY(upload4(R, p));
  res->envelope_entries = R.P.env_entries;
  res->envelope_tiles = R.P.ntiles;
  res->tall_columns = R.P.tall;
  // computeLambdaInit: the user's value, else tau * max diag(H), tau = kLmTau
  auto lambda0 = [&](double* l) {
    if (p->lambda_init > 0) { *l = p->lambda_init; return OSH_OK; }
    double maxd = 0;
    OSH_TRY(R.max_diag(&maxd));
    *l = kLmTau * maxd;
    return OSH_OK;
  };
  LmResult lm;
  OSH_TRY(R.solve(p->iterations, lambda0, lm));
  const size_t n = p->n_vertices;
  std::vector<double> st(n * kStateDoubles);
  OSH_HIP(hipMemcpyAsync(st.data(), R.d_x[lm.cur], st.size() * 8, hipMemcpyDeviceToHost, R.s));
  OSH_HIP(hipStreamSynchronize(R.s));
  for (size_t v = 0; v < n; ++v) {
    const double* o = st.data() + v * kStateDoubles;
    for (int k = 0; k < 9; ++k) res->Rcw[9 * v + k] = o[21 + k];
    for (int k = 0; k < 3; ++k) res->tcw[3 * v + k] = o[30 + k];
    if (res->Rwb) for (int k = 0; k < 9; ++k) res->Rwb[9 * v + k] = o[9 + k];
    if (res->twb) for (int k = 0; k < 3; ++k) res->twb[3 * v + k] = o[18 + k];
  }
  res->iterations = lm.iterations;
  res->trials = lm.trials;
  res->chi2_initial = lm.chi2_initial;
  res->chi2_final = lm.chi2_final;
  res->lambda_init_used = lm.lambda0;
  res->status = OSH_OK;
  return OSH_OK;
}

extern "C" int osh_pgo4_linearize(osh_lba_ctx* ctx, const osh_pgo4_problem* p, double* H, double* b, double* chi2) {
  if (!ctx || !H || !b || !chi2) { set_error("osh_pgo4_linearize: bad arguments"); return OSH_ERR_INVALID; }
  Run4 R(ctx);
  OSH_TRY(check4(R, p));
  OSH_TRY(R.dense_fits());
  OSH_TRY(upload4(R, p));
  return R.linearize(H, b, chi2);
}
