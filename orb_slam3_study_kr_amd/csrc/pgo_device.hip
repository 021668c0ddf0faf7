// pgo_device.hip -- the Sim3 pose graph of Optimizer::OptimizeEssentialGraph on the device (include/orbslam3_hip.h,
// osh_pgo_*).  One VertexSim3Expmap per keyframe, EdgeSim3 with identity information, g2o's central-difference Jacobians,
// Levenberg-Marquardt as optimization_algorithm_levenberg.cpp:99-169 runs it (the controller stays on the host: one
// three-double read-back per trial).
//
// Kernels, in the order of one trial:
//   k_pgo_lin       thread per edge: error and the two 7x7 numeric Jacobians (delta 1e-9, push / oplus / pop), at linearisation
//   k_pgo_assemble  block per 7x7 block of H: sums its edges in edge order (CSR built at upload, no atomics); b = -J^T e
//   k_pgo_fill      H + lambda I into the envelope tiles of the working matrix, b into the right-hand side
//   k_env_diag / k_env_panel / k_env_update    right-looking LDL^T (A = U^T D U, upper storage) in 32-wide panels over the
//                   column envelope: panel p touches only the column tiles whose envelope reaches row tile p (the active list),
//                   the trailing update runs on the FP64 matrix cores over pairs of active tiles
//   k_env_back      x = U^-1 w, panels in reverse, each panel row dotted with its active tiles only
//   k_pgo_step      estimate' = exp(x_v) * estimate for every free vertex
//   k_pgo_err       error of every edge at estimate'; k_pgo_reduce: chi2 and computeScale in a fixed order
//
// The envelope storage, the LDL^T kernels, the reduction and the plan are shared with the 4-DoF graph (pgo_env.h).  Spanning-
// tree and covisibility edges sit near the diagonal; a loop edge makes the columns of its newer keyframe tall.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <vector>
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

struct AsmView {
  const double* J; const double* err;
  const int* blk_a; const int* blk_b;     // [nblk] free-vertex indices (a == b: diagonal block), a <= b
  const int* ent_ptr; const int* ent;     // [nblk + 1], entries: diagonal (e << 1 | side), off-diagonal (e << 1 | flip)
  double* H;                              // [nblk][49]
  double* b;                              // [7 nf]
  int nblk;
};

__global__ __launch_bounds__(64) void k_pgo_assemble(AsmView v) {
  const int k = blockIdx.x, t = threadIdx.x;
  const int a = v.blk_a[k], bb = v.blk_b[k];
  const int p0 = v.ent_ptr[k], p1 = v.ent_ptr[k + 1];
  if (t < 49) {
    const int r = t / 7, c = t - 7 * (t / 7);
    double s = 0;
    for (int q = p0; q < p1; ++q) {
      const int en = v.ent[q], e = en >> 1, f = en & 1;
      const double* Ja;
      const double* Jb;
      if (a == bb) { Ja = Jb = v.J + ((size_t)e * 2 + f) * 49; }
      else { Ja = v.J + ((size_t)e * 2 + f) * 49; Jb = v.J + ((size_t)e * 2 + (1 - f)) * 49; }
      double h = 0;
      for (int m = 0; m < 7; ++m) h += Ja[m * 7 + r] * Jb[m * 7 + c];
      s += h;
    }
    v.H[(size_t)k * 49 + t] = s;
  } else if (a == bb && t < 56) {
    const int r = t - 49;
    double s = 0;
    for (int q = p0; q < p1; ++q) {
      const int en = v.ent[q], e = en >> 1, f = en & 1;
      const double* Ja = v.J + ((size_t)e * 2 + f) * 49;
      const double* er = v.err + 7 * (size_t)e;
      double h = 0;
      for (int m = 0; m < 7; ++m) h += Ja[m * 7 + r] * er[m];
      s -= h;
    }
    v.b[7 * a + r] = s;
  }
}

__global__ __launch_bounds__(64) void k_pgo_fill(AsmView v, Env g, double lambda, int nf) {
  const int k = blockIdx.x, t = threadIdx.x;
  if (k == v.nblk) {   // padding of the last tile: identity, zero rhs
    for (int R = 7 * nf + t; R < kT * g.NT; R += 64) { env_tile(g, R >> 5, R >> 5)[(R & 31) * kT + (R & 31)] = 1.0; g.w[R] = 0.0; }
    return;
  }
  const int a = v.blk_a[k], bb = v.blk_b[k];
  if (t < 49) {
    const int r = t / 7, c = t - 7 * (t / 7);
    const int R = 7 * a + r, Cc = 7 * bb + c;
    if (R <= Cc) {
      double h = v.H[(size_t)k * 49 + t];
      if (R == Cc) h += lambda;
      env_tile(g, R >> 5, Cc >> 5)[(R & 31) * kT + (Cc & 31)] = h;
    }
  } else if (a == bb && t < 56) {
    g.w[7 * a + t - 49] = v.b[7 * a + t - 49];
  }
}

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

// Everything of one call on the device: upload, linearisation, and the LM loop when `res` is given.
struct Run {
  osh_lba_ctx* ctx;
  hipStream_t s = nullptr;
  PgoBuffers* B = nullptr;
  Plan P;
  double *d_est[2] = {nullptr, nullptr}, *d_meas, *d_J, *d_err, *d_chi, *d_H, *d_b, *d_w, *d_z, *d_red;
  int *d_eij, *d_sys, *d_blk_a, *d_blk_b, *d_ent_ptr, *d_ent, *d_toff, *d_ttop, *d_act_ptr, *d_act, *d_fail;
  unsigned char* d_fixs;
  double* h_red = nullptr;

  int setup(const osh_pgo_problem* p) {
    OSH_TRY(validate(p));
    OSH_TRY(make_plan(PlanInput{p->n_vertices, p->n_edges, p->solve_mode, p->fixed, p->edge_ij}, 7, "osh_pgo", P));   // size checks before any device work
    int device = 0;
    OSH_TRY(lba_stream(ctx, &device, &s));
    OSH_HIP(hipSetDevice(device));
    void** slot = lba_attachment(ctx, kAttachPgo, [](void* q) { delete static_cast<PgoBuffers*>(q); });
    if (!slot) { set_error("osh_pgo: no context"); return OSH_ERR_INVALID; }
    if (!*slot) *slot = new PgoBuffers();
    B = static_cast<PgoBuffers*>(*slot);
    const size_t n = P.n, E = std::max(P.E, 1), NT = P.NT;
    size_t bytes = 0;
    auto take = [&](size_t b) { const size_t o = bytes; bytes = (bytes + std::max<size_t>(b, 8) + 255) & ~(size_t)255; return o; };
    const size_t o_est0 = take(n * 64), o_est1 = take(n * 64), o_meas = take(E * 64), o_J = take(E * 2 * 49 * 8), o_err = take(E * 56),
                 o_chi = take(E * 8), o_H = take((size_t)P.nblk * 49 * 8), o_b = take((size_t)P.N * 8 + 8), o_w = take(NT * kT * 8),
                 o_z = take(NT * kT * 8), o_red = take(64), o_eij = take(E * 8), o_sys = take(n * 4), o_blk_a = take((size_t)P.nblk * 4),
                 o_blk_b = take((size_t)P.nblk * 4), o_ent_ptr = take((size_t)(P.nblk + 1) * 4), o_ent = take(P.ent.size() * 4 + 4),
                 o_toff = take(NT * 4), o_ttop = take(NT * 4), o_act_ptr = take((NT + 1) * 4), o_act = take(P.act.size() * 4),
                 o_fail = take(4), o_fixs = take(n);
    OSH_TRY(B->arena.reserve(bytes));
    OSH_TRY(B->tiles.reserve((size_t)P.ntiles * kTT * 8));
    OSH_TRY(B->V.reserve((size_t)P.max_act * kTT * 8));
    h_red = static_cast<double*>(B->h_red.reserve(64));
    if (!h_red) { set_error("osh_pgo: pinned allocation failed"); return OSH_ERR_DEVICE; }
    char* base = B->arena.as<char>();
    d_est[0] = (double*)(base + o_est0); d_est[1] = (double*)(base + o_est1); d_meas = (double*)(base + o_meas);
    d_J = (double*)(base + o_J); d_err = (double*)(base + o_err); d_chi = (double*)(base + o_chi); d_H = (double*)(base + o_H);
    d_b = (double*)(base + o_b); d_w = (double*)(base + o_w); d_z = (double*)(base + o_z); d_red = (double*)(base + o_red);
    d_eij = (int*)(base + o_eij); d_sys = (int*)(base + o_sys); d_blk_a = (int*)(base + o_blk_a); d_blk_b = (int*)(base + o_blk_b);
    d_ent_ptr = (int*)(base + o_ent_ptr); d_ent = (int*)(base + o_ent); d_toff = (int*)(base + o_toff); d_ttop = (int*)(base + o_ttop);
    d_act_ptr = (int*)(base + o_act_ptr); d_act = (int*)(base + o_act); d_fail = (int*)(base + o_fail); d_fixs = (unsigned char*)(base + o_fixs);
    // Jacobians of fixed sides are never written or read; zero the arena once per call so that nothing depends on its history
    OSH_HIP(hipMemsetAsync(base, 0, bytes, s));
    auto up = [&](void* d, const void* h, size_t b) -> int { if (b) OSH_HIP(hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, s)); return OSH_OK; };
    OSH_TRY(up(d_est[0], p->estimate, n * 64));
    OSH_TRY(up(d_meas, p->measurement, (size_t)P.E * 64));
    OSH_TRY(up(d_eij, p->edge_ij, (size_t)P.E * 8));
    OSH_TRY(up(d_sys, P.sys.data(), n * 4));
    OSH_TRY(up(d_fixs, p->fix_scale, n));
    OSH_TRY(up(d_blk_a, P.blk_a.data(), (size_t)P.nblk * 4));
    OSH_TRY(up(d_blk_b, P.blk_b.data(), (size_t)P.nblk * 4));
    OSH_TRY(up(d_ent_ptr, P.ent_ptr.data(), (size_t)(P.nblk + 1) * 4));
    OSH_TRY(up(d_ent, P.ent.data(), P.ent.size() * 4));
    OSH_TRY(up(d_toff, P.toff.data(), NT * 4));
    OSH_TRY(up(d_ttop, P.ttop.data(), NT * 4));
    OSH_TRY(up(d_act_ptr, P.act_ptr.data(), (NT + 1) * 4));
    OSH_TRY(up(d_act, P.act.data(), P.act.size() * 4));
    return OSH_OK;
  }

  PgoView view(int cur) const {
    PgoView v;
    v.est = d_est[cur]; v.eij = d_eij; v.meas = d_meas; v.sys = d_sys; v.fixs = d_fixs; v.J = d_J; v.err = d_err; v.chi = d_chi; v.E = P.E;
    return v;
  }
  AsmView asm_view() const {
    AsmView a;
    a.J = d_J; a.err = d_err; a.blk_a = d_blk_a; a.blk_b = d_blk_b; a.ent_ptr = d_ent_ptr; a.ent = d_ent; a.H = d_H; a.b = d_b; a.nblk = P.nblk;
    return a;
  }
  Env env() const {
    Env g;
    g.T = B->tiles.as<double>(); g.toff = d_toff; g.ttop = d_ttop; g.act_ptr = d_act_ptr; g.act = d_act; g.V = B->V.as<double>();
    g.w = d_w; g.z = d_z; g.fail = d_fail; g.NT = P.NT;
    return g;
  }

  // errors (and Jacobians) at d_est[cur]; returns chi2 through the read-back
  int errors(int cur, int linearize) {
    if (P.E > 0) hipLaunchKernelGGL(k_pgo_lin, dim3((unsigned)((P.E + 63) / 64)), dim3(64), 0, s, view(cur), linearize);
    return launch_check("k_pgo_lin");
  }
  int assemble() {
    if (P.nblk > 0) hipLaunchKernelGGL(k_pgo_assemble, dim3((unsigned)P.nblk), dim3(64), 0, s, asm_view());
    return launch_check("k_pgo_assemble");
  }
  // one trial: (H + lambda I) x = b into d_w, d_est[1 - cur] = x (+) d_est[cur]; chi2 and the scale into h_red
  int trial(int cur, double lambda) {
    const Env g = env();
    OSH_HIP(hipMemsetAsync(d_fail, 0, 4, s));
    OSH_HIP(hipMemsetAsync(B->tiles.p, 0, (size_t)P.ntiles * kTT * 8, s));
    hipLaunchKernelGGL(k_pgo_fill, dim3((unsigned)P.nblk + 1), dim3(64), 0, s, asm_view(), g, lambda, P.nf);
    OSH_TRY(launch_check("k_pgo_fill"));
    for (int q = 0; q < P.NT; ++q) {
      hipLaunchKernelGGL(k_env_diag, dim3(1), dim3(64), 0, s, g, q);
      const int na = P.act_ptr[q + 1] - P.act_ptr[q];
      if (na > 0) {
        hipLaunchKernelGGL(k_env_panel, dim3((unsigned)na), dim3(64), 0, s, g, q);
        hipLaunchKernelGGL(k_env_update, dim3((unsigned)na, (unsigned)na), dim3(64), 0, s, g, q);
      }
    }
    OSH_TRY(launch_check("k_env_factor"));
    hipLaunchKernelGGL(k_env_back, dim3(1), dim3(1024), 0, s, g);
    hipLaunchKernelGGL(k_pgo_step, dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, s, d_est[cur], d_est[1 - cur], d_sys, d_fixs, d_w, d_fail, P.n);
    OSH_TRY(launch_check("k_pgo_step"));
    OSH_TRY(errors(1 - cur, 0));
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(1024), 0, s, d_chi, P.E, d_w, d_b, P.N, lambda, 1, d_red);
    OSH_TRY(launch_check("k_pgo_reduce"));
    OSH_HIP(hipMemcpyAsync(d_red + 2, d_fail, 4, hipMemcpyDeviceToDevice, s));
    OSH_HIP(hipMemcpyAsync(h_red, d_red, 24, hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
    return OSH_OK;
  }
  int chi2_now(double* out) {
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(1024), 0, s, d_chi, P.E, d_w, d_b, 0, 0.0, 0, d_red);
    OSH_TRY(launch_check("k_pgo_reduce"));
    OSH_HIP(hipMemcpyAsync(h_red, d_red, 16, hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
    *out = h_red[0];
    return OSH_OK;
  }
};

}  // namespace
}  // namespace osh

using namespace osh;

extern "C" int osh_pgo_solve(osh_lba_ctx* ctx, const osh_pgo_problem* p, osh_pgo_result* res) {
  if (!ctx || !res) { set_error("osh_pgo_solve: bad arguments"); return OSH_ERR_INVALID; }
  res->status = OSH_ERR_INVALID;
  Run R;
  R.ctx = ctx;
  {
    const int rc = R.setup(p);
    if (rc != OSH_OK) { res->status = rc; return rc; }
  }
  if (!(p->lambda_init > 0)) { set_error("osh_pgo_solve: lambda_init must be > 0"); return OSH_ERR_INVALID; }
  res->envelope_entries = R.P.env_entries;
  res->envelope_tiles = R.P.ntiles;
  res->tall_columns = R.P.tall;
  // SparseOptimizer::optimize (sparse_optimizer.cpp:354-419) with OptimizationAlgorithmLevenberg::solve (levenberg.cpp:99-169)
  int cur = 0, iterations = 0, trials = 0, nBad = 0;
  double lambda = p->lambda_init, ni = 2.0, chi2_initial = 0.0;
  const int maxTrials = 10;
  bool ok = true;
  for (int it = 0; it < p->iterations && ok; ++it) {
    OSH_TRY(R.errors(cur, 1));
    double currentChi = 0;
    OSH_TRY(R.chi2_now(&currentChi));
    if (it == 0) chi2_initial = currentChi;
    const double iniChi = currentChi;
    OSH_TRY(R.assemble());
    if (it == 0) { lambda = p->lambda_init; ni = 2; nBad = 0; }
    double rho = 0;
    int qmax = 0;
    do {
      OSH_TRY(R.trial(cur, lambda));
      double tempChi = R.h_red[0];
      const double scale = R.h_red[1] + 1e-3;
      int fail = 0;
      std::memcpy(&fail, &R.h_red[2], 4);
      if (fail) tempChi = std::numeric_limits<double>::max();
      rho = (currentChi - tempChi) / scale;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        const double scaleFactor = std::max(1. / 3., alpha);
        lambda *= scaleFactor;
        ni = 2;
        currentChi = tempChi;
        cur = 1 - cur;   // discardTop: the trial's estimates become the state
      } else {
        lambda *= ni;
        ni *= 2;         // pop: the trial's estimates are dropped
      }
      ++qmax;
      ++trials;
    } while (rho < 0 && qmax < maxTrials);
    ++iterations;
    if (qmax == maxTrials || rho == 0) { ok = false; continue; }
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;   // the stop rule of this g2o copy (levenberg.cpp:154-164)
    if (nBad >= 3) ok = false;
  }
  // computeActiveErrors at the returned estimates
  OSH_TRY(R.errors(cur, 0));
  double chi2_final = 0;
  OSH_TRY(R.chi2_now(&chi2_final));
  if (p->n_vertices > 0 && res->estimate) {
    OSH_HIP(hipMemcpyAsync(res->estimate, R.d_est[cur], (size_t)p->n_vertices * 64, hipMemcpyDeviceToHost, R.s));
    OSH_HIP(hipStreamSynchronize(R.s));
  }
  res->iterations = iterations;
  res->trials = trials;
  res->chi2_initial = chi2_initial;
  res->chi2_final = chi2_final;
  res->status = OSH_OK;
  return OSH_OK;
}

extern "C" int osh_pgo_linearize(osh_lba_ctx* ctx, const osh_pgo_problem* p, double* H, double* b, double* chi2) {
  if (!ctx || !H || !b || !chi2) { set_error("osh_pgo_linearize: bad arguments"); return OSH_ERR_INVALID; }
  Run R;
  R.ctx = ctx;
  OSH_TRY(R.setup(p));
  if (R.P.nf > 512) { set_error("osh_pgo_linearize: %d free vertices, the diagnostic takes up to 512", R.P.nf); return OSH_ERR_UNSUPPORTED; }
  OSH_TRY(R.errors(0, 1));
  OSH_TRY(R.chi2_now(chi2));
  OSH_TRY(R.assemble());
  std::vector<double> blocks((size_t)R.P.nblk * 49);
  if (!blocks.empty()) OSH_HIP(hipMemcpyAsync(blocks.data(), R.d_H, blocks.size() * 8, hipMemcpyDeviceToHost, R.s));
  if (R.P.N > 0) OSH_HIP(hipMemcpyAsync(b, R.d_b, (size_t)R.P.N * 8, hipMemcpyDeviceToHost, R.s));
  OSH_HIP(hipStreamSynchronize(R.s));
  const size_t N = R.P.N;
  std::fill(H, H + N * N, 0.0);
  for (int k = 0; k < R.P.nblk; ++k) {
    const int a = R.P.blk_a[k], bb = R.P.blk_b[k];
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) {
        const double h = blocks[(size_t)k * 49 + r * 7 + c];
        H[(size_t)(7 * a + r) * N + 7 * bb + c] = h;
        if (a != bb) H[(size_t)(7 * bb + c) * N + 7 * a + r] = h;
      }
  }
  return OSH_OK;
}
