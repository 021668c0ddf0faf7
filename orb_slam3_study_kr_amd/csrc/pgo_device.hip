// pgo_device.hip -- the Sim3 pose graph of Optimizer::OptimizeEssentialGraph on the device (include/orbslam3_hip.h,
// osh_pgo_*).  One VertexSim3Expmap per keyframe, EdgeSim3 with identity information, g2o's central-difference Jacobians,
// Levenberg-Marquardt as optimization_algorithm_levenberg.cpp:99-169 runs it (the controller stays on the host: one
// three-double read-back per trial).
//
// Kernels, in the order of one trial:
//   k_pgo_lin       thread per edge: error and the two 7x7 numeric Jacobians (delta 1e-9, push / oplus / pop), at linearisation
//   k_pgo_assemble  block per 7x7 block of H: sums its edges in edge order (CSR built at upload, no atomics); b = -J^T e
//                   (pgo_env.h, with the identity information)
//   k_pgo_fill      H + lambda I into the envelope tiles of the working matrix, b into the right-hand side (pgo_env.h)
//   k_env_diag / k_env_panel / k_env_update    right-looking LDL^T (A = U^T D U, upper storage) in 32-wide panels over the
//                   column envelope: panel p touches only the column tiles whose envelope reaches row tile p (the active list),
//                   the trailing update runs on the FP64 matrix cores over pairs of active tiles
//   k_env_back      x = U^-1 w, panels in reverse, each panel row dotted with its active tiles only
//   k_pgo_step      estimate' = exp(x_v) * estimate for every free vertex
//   k_pgo_lin (errors only) at estimate'; k_pgo_reduce: chi2 and computeScale in a fixed order
//
// This file holds the Sim3 vertex and edge (Sim3Graph): k_pgo_lin, k_pgo_step, the validation, the upload of the caller's
// estimates and the write-back.  The envelope storage, the LDL^T kernels, the reduction, the plan, the
// trial sequence and the LM loop are shared with the 4-DoF graph (pgo_env.h).  Spanning-tree and covisibility edges sit near
// the diagonal; a loop edge makes the columns of its newer keyframe tall.
#include <hip/hip_runtime.h>
#include "common.h"
#include "pgo_env.h"
#include "pgo_sim3.h"

namespace osh {
namespace {

struct PgoView {
  const double* est;              // [n][8] estimates the edges are evaluated at
  const int* eij;                 // [E][2]
  const double* meas;             // [E][8]
  const int* sys;                 // [n] index of the free vertex, -1 when fixed
  const unsigned char* fixs;      // [n] _fix_scale
  double* J;                      // [E][2][49]  d e_r / d x_c, row-major
  double* err;                    // [E][7]
  double* chi;                    // [E]
  int E;
};

__global__ __launch_bounds__(64) void k_pgo_lin(PgoView v, int linearize) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= v.E) return;
  using namespace pgo;
  const int vi = v.eij[2 * e], vj = v.eij[2 * e + 1];
  const Sim3 C = sim3_load(v.meas + 8 * (size_t)e), Si = sim3_load(v.est + 8 * (size_t)vi), Sj = sim3_load(v.est + 8 * (size_t)vj);
  double e0[7];
  edge_error(C, Si, Sj, e0);
  double c2 = 0;
  for (int k = 0; k < 7; ++k) { v.err[7 * (size_t)e + k] = e0[k]; c2 += e0[k] * e0[k]; }
  v.chi[e] = c2;
  if (!linearize) return;
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  for (int side = 0; side < 2; ++side) {
    const int vx = side ? vj : vi;
    if (v.sys[vx] < 0) continue;
    const bool fs = v.fixs[vx] != 0;
    const Sim3 X = side ? Sj : Si;
    double* Jo = v.J + ((size_t)e * 2 + side) * 49;
    for (int d = 0; d < 7; ++d) {
      double add[7] = {0, 0, 0, 0, 0, 0, 0}, ep[7], em[7];
      add[d] = delta;
      const Sim3 Xp = vertex_oplus(X, add, fs);
      if (side) edge_error(C, Si, Xp, ep); else edge_error(C, Xp, Sj, ep);
      add[d] = -delta;
      const Sim3 Xm = vertex_oplus(X, add, fs);
      if (side) edge_error(C, Si, Xm, em); else edge_error(C, Xm, Sj, em);
      for (int r = 0; r < 7; ++r) { double bak = ep[r]; bak -= em[r]; Jo[r * 7 + d] = scalar * bak; }
    }
  }
}

struct AsmView : AsmArrays {
  int nblk;
};

__global__ __launch_bounds__(256) void k_pgo_step(const double* est, double* est_new, const int* sys, const unsigned char* fixs,
                                                  const double* x, const int* fail, int n) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int a = sys[v];
  if (a < 0 || *fail) {
    for (int k = 0; k < 8; ++k) est_new[8 * (size_t)v + k] = est[8 * (size_t)v + k];
    return;
  }
  const pgo::Sim3 s = pgo::vertex_oplus(pgo::sim3_load(est + 8 * (size_t)v), x + 7 * (size_t)a, fixs[v] != 0);
  pgo::sim3_store(s, est_new + 8 * (size_t)v);
}

int validate(const osh_pgo_problem* p) {
  if (!p || p->n_vertices <= 0 || p->n_edges < 0 || !p->estimate || !p->fixed || !p->fix_scale ||
      (p->n_edges > 0 && (!p->edge_ij || !p->measurement))) {
    set_error("osh_pgo: bad problem (sizes or NULL arrays)");
    return OSH_ERR_INVALID;
  }
  if (p->solve_mode != OSH_PGO_SOLVE_ENVELOPE && p->solve_mode != OSH_PGO_SOLVE_DENSE) { set_error("osh_pgo: unknown solve_mode"); return OSH_ERR_INVALID; }
  return OSH_OK;
}

struct Sim3Graph {
  static constexpr int D = 7, M = 7, kState = 8, kMeas = 8, kAux = 1;
  static constexpr bool kDiagInfo = false;
  using Aux = unsigned char;   // _fix_scale
  static constexpr const char* kTag = "osh_pgo";

  template <class R> AsmView asm_view(const R& r) const { return AsmView{r.asm_arrays(), r.P.nblk}; }
  template <class R> int lin(const R& r, int cur, int linearize) const {
    PgoView v;
    v.est = r.d_x[cur]; v.eij = r.d_eij; v.meas = r.d_meas; v.sys = r.d_sys; v.fixs = r.d_aux; v.J = r.d_J; v.err = r.d_err;
    v.chi = r.d_chi; v.E = r.P.E;
    if (r.P.E > 0) hipLaunchKernelGGL(k_pgo_lin, dim3((unsigned)((r.P.E + 63) / 64)), dim3(64), 0, r.s, v, linearize);
    return launch_check("k_pgo_lin");
  }
  template <class R> int step(const R& r, int cur) const {
    hipLaunchKernelGGL(k_pgo_step, dim3((unsigned)((r.P.n + 255) / 256)), dim3(256), 0, r.s, r.d_x[cur], r.d_x[1 - cur], r.d_sys, r.d_aux,
                       r.d_w, r.d_fail, r.P.n);
    return launch_check("k_pgo_step");
  }
};

using Run = PgoRun<Sim3Graph>;

// validation and the plan: no device work
int check(Run& R, const osh_pgo_problem* p) {
  OSH_TRY(validate(p));
  return R.plan(PlanInput{p->n_vertices, p->n_edges, p->solve_mode, p->fixed, p->edge_ij});
}

int upload(Run& R, const osh_pgo_problem* p) { return R.upload(p->estimate, p->measurement, p->edge_ij, p->fix_scale); }

}  // namespace
}  // namespace osh

using namespace osh;

extern "C" int osh_pgo_solve(osh_lba_ctx* ctx, const osh_pgo_problem* p, osh_pgo_result* res) {
  if (!ctx || !res) { set_error("osh_pgo_solve: bad arguments"); return OSH_ERR_INVALID; }
  res->status = OSH_ERR_INVALID;
  Run R(ctx);
  int rc = check(R, p);
  if (rc == OSH_OK && !(p->lambda_init > 0)) { set_error("osh_pgo_solve: lambda_init must be > 0"); rc = OSH_ERR_INVALID; }
  if (rc == OSH_OK) rc = upload(R, p);
  if (rc != OSH_OK) { res->status = rc; return rc; }
  res->envelope_entries = R.P.env_entries;
  res->envelope_tiles = R.P.ntiles;
  res->tall_columns = R.P.tall;
  LmResult lm;
  OSH_TRY(R.solve(p->iterations, [&](double* l) { *l = p->lambda_init; return OSH_OK; }, lm));
  if (p->n_vertices > 0 && res->estimate) {
    OSH_HIP(hipMemcpyAsync(res->estimate, R.d_x[lm.cur], (size_t)p->n_vertices * 64, hipMemcpyDeviceToHost, R.s));
    OSH_HIP(hipStreamSynchronize(R.s));
  }
  res->iterations = lm.iterations;
  res->trials = lm.trials;
  res->chi2_initial = lm.chi2_initial;
  res->chi2_final = lm.chi2_final;
  res->status = OSH_OK;
  return OSH_OK;
}

extern "C" int osh_pgo_linearize(osh_lba_ctx* ctx, const osh_pgo_problem* p, double* H, double* b, double* chi2) {
  if (!ctx || !H || !b || !chi2) { set_error("osh_pgo_linearize: bad arguments"); return OSH_ERR_INVALID; }
  Run R(ctx);
  OSH_TRY(check(R, p));
  OSH_TRY(R.dense_fits());
  OSH_TRY(upload(R, p));
  return R.linearize(H, b, chi2);
}
