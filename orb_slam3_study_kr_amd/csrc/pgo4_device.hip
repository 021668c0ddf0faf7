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
//   k_pgo4_assemble  block per 4x4 block of H: sums its edges in edge order (CSR built at upload, no atomics); b = -J^T Omega e
//   k_pgo4_maxdiag   once, when lambda_0 is g2o's: max |diag H| over the free vertices
//   k_pgo4_fill      H + lambda I into the envelope tiles (8 vertices per 32-wide tile), b into the right-hand side
//   k_env_*          the Sim3 graph's envelope LDL^T, unchanged (pgo_env.h)
//   k_pgo4_step      UpdateW of every free vertex into the candidate state
//   k_pgo4_lin (errors only) and k_pgo_reduce: chi2 and computeScale in a fixed order
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
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

struct Asm4View {
  const double* J; const double* err;
  const int* blk_a; const int* blk_b;     // [nblk] free-vertex indices (a == b: diagonal block), a <= b
  const int* ent_ptr; const int* ent;     // [nblk + 1], entries: diagonal (e << 1 | side), off-diagonal (e << 1 | flip)
  double* H;                              // [nblk][16]
  double* b;                              // [4 nf]
  Info6 info;
  int nblk;
};

__global__ __launch_bounds__(64) void k_pgo4_assemble(Asm4View v) {
  const int k = blockIdx.x, t = threadIdx.x;
  const int a = v.blk_a[k], bb = v.blk_b[k];
  const int p0 = v.ent_ptr[k], p1 = v.ent_ptr[k + 1];
  if (t < 16) {
    const int r = t >> 2, c = t & 3;
    double s = 0;
    for (int q = p0; q < p1; ++q) {
      const int en = v.ent[q], e = en >> 1, f = en & 1;
      const double* Ja = v.J + ((size_t)e * 2 + f) * 24;
      const double* Jb = a == bb ? Ja : v.J + ((size_t)e * 2 + (1 - f)) * 24;
      double h = 0;
      for (int m = 0; m < 6; ++m) h += (Ja[m * 4 + r] * v.info.w[m]) * Jb[m * 4 + c];
      s += h;
    }
    v.H[(size_t)k * 16 + t] = s;
  } else if (a == bb && t < 20) {
    const int r = t - 16;
    double s = 0;
    for (int q = p0; q < p1; ++q) {
      const int en = v.ent[q], e = en >> 1, f = en & 1;
      const double* Ja = v.J + ((size_t)e * 2 + f) * 24;
      const double* er = v.err + 6 * (size_t)e;
      double h = 0;
      for (int m = 0; m < 6; ++m) h += (Ja[m * 4 + r] * v.info.w[m]) * er[m];
      s -= h;
    }
    v.b[4 * a + r] = s;
  }
}

// max |H_kk| over the diagonal blocks 0 .. nf-1 (they come first in the block list); max is exact in any order
__global__ __launch_bounds__(256) void k_pgo4_maxdiag(const double* H, int nf, double* out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double m = 0.0;
  for (int k = t; k < 4 * nf; k += 256) m = fmax(m, fabs(H[(size_t)(k >> 2) * 16 + (k & 3) * 5]));
  red[t] = m;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] = fmax(red[t], red[t + h]);
    __syncthreads();
  }
  if (t == 0) *out = red[0];
}

__global__ __launch_bounds__(64) void k_pgo4_fill(Asm4View v, Env g, double lambda, int nf) {
  const int k = blockIdx.x, t = threadIdx.x;
  if (k == v.nblk) {   // padding of the last tile: identity, zero rhs
    for (int R = 4 * nf + t; R < kT * g.NT; R += 64) { env_tile(g, R >> 5, R >> 5)[(R & 31) * kT + (R & 31)] = 1.0; g.w[R] = 0.0; }
    return;
  }
  const int a = v.blk_a[k], bb = v.blk_b[k];
  if (t < 16) {
    const int r = t >> 2, c = t & 3;
    const int R = 4 * a + r, Cc = 4 * bb + c;
    if (R <= Cc) {
      double h = v.H[(size_t)k * 16 + t];
      if (R == Cc) h += lambda;
      env_tile(g, R >> 5, Cc >> 5)[(R & 31) * kT + (Cc & 31)] = h;
    }
  } else if (a == bb && t < 20) {
    g.w[4 * a + t - 16] = v.b[4 * a + t - 16];
  }
}

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

// Everything of one call on the device: upload, linearisation, and the LM loop.
struct Run4 {
  osh_lba_ctx* ctx;
  hipStream_t s = nullptr;
  PgoBuffers* B = nullptr;
  Plan P;
  Info6 info;
  double *d_st[2] = {nullptr, nullptr}, *d_cst, *d_meas, *d_J, *d_err, *d_chi, *d_H, *d_b, *d_w, *d_z, *d_red;
  int *d_eij, *d_sys, *d_blk_a, *d_blk_b, *d_ent_ptr, *d_ent, *d_toff, *d_ttop, *d_act_ptr, *d_act, *d_fail;
  double* h_red = nullptr;

  // validation and the plan only: no device work
  int check(const osh_pgo4_problem* p) {
    OSH_TRY(validate4(p));
    return make_plan(PlanInput{p->n_vertices, p->n_edges, p->solve_mode, p->fixed, p->edge_ij}, 4, "osh_pgo4", P);
  }

  int setup(const osh_pgo4_problem* p) {
    for (int k = 0; k < 6; ++k) info.w[k] = p->info_diag[k];
    int device = 0;
    OSH_TRY(lba_stream(ctx, &device, &s));
    OSH_HIP(hipSetDevice(device));
    void** slot = lba_attachment(ctx, kAttachPgo, [](void* q) { delete static_cast<PgoBuffers*>(q); });
    if (!slot) { set_error("osh_pgo4: no context"); return OSH_ERR_INVALID; }
    if (!*slot) *slot = new PgoBuffers();
    B = static_cast<PgoBuffers*>(*slot);
    const size_t n = P.n, E = std::max(P.E, 1), NT = P.NT;
    size_t bytes = 0;
    auto take = [&](size_t b) { const size_t o = bytes; bytes = (bytes + std::max<size_t>(b, 8) + 255) & ~(size_t)255; return o; };
    const size_t o_st0 = take(n * kStateDoubles * 8), o_st1 = take(n * kStateDoubles * 8), o_cst = take(n * kConstDoubles * 8),
                 o_meas = take(E * 12 * 8), o_J = take(E * 2 * 24 * 8), o_err = take(E * 6 * 8), o_chi = take(E * 8),
                 o_H = take((size_t)P.nblk * 16 * 8), o_b = take((size_t)P.N * 8 + 8), o_w = take(NT * kT * 8), o_z = take(NT * kT * 8),
                 o_red = take(64), o_eij = take(E * 8), o_sys = take(n * 4), o_blk_a = take((size_t)P.nblk * 4),
                 o_blk_b = take((size_t)P.nblk * 4), o_ent_ptr = take((size_t)(P.nblk + 1) * 4), o_ent = take(P.ent.size() * 4 + 4),
                 o_toff = take(NT * 4), o_ttop = take(NT * 4), o_act_ptr = take((NT + 1) * 4), o_act = take(P.act.size() * 4),
                 o_fail = take(4);
    OSH_TRY(B->arena.reserve(bytes));
    OSH_TRY(B->tiles.reserve((size_t)P.ntiles * kTT * 8));
    OSH_TRY(B->V.reserve((size_t)P.max_act * kTT * 8));
    h_red = static_cast<double*>(B->h_red.reserve(64));
    if (!h_red) { set_error("osh_pgo4: pinned allocation failed"); return OSH_ERR_DEVICE; }
    char* base = B->arena.as<char>();
    d_st[0] = (double*)(base + o_st0); d_st[1] = (double*)(base + o_st1); d_cst = (double*)(base + o_cst); d_meas = (double*)(base + o_meas);
    d_J = (double*)(base + o_J); d_err = (double*)(base + o_err); d_chi = (double*)(base + o_chi); d_H = (double*)(base + o_H);
    d_b = (double*)(base + o_b); d_w = (double*)(base + o_w); d_z = (double*)(base + o_z); d_red = (double*)(base + o_red);
    d_eij = (int*)(base + o_eij); d_sys = (int*)(base + o_sys); d_blk_a = (int*)(base + o_blk_a); d_blk_b = (int*)(base + o_blk_b);
    d_ent_ptr = (int*)(base + o_ent_ptr); d_ent = (int*)(base + o_ent); d_toff = (int*)(base + o_toff); d_ttop = (int*)(base + o_ttop);
    d_act_ptr = (int*)(base + o_act_ptr); d_act = (int*)(base + o_act); d_fail = (int*)(base + o_fail);
    // the initial vertex states (DR = I, its = 0, the raw camera pose) and the constants, packed on the host
    std::vector<double> st(n * kStateDoubles), cst(n * kConstDoubles), meas((size_t)P.E * 12);
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
    for (int e = 0; e < P.E; ++e) {
      for (int k = 0; k < 9; ++k) meas[12 * (size_t)e + k] = p->dR[9 * (size_t)e + k];
      for (int k = 0; k < 3; ++k) meas[12 * (size_t)e + 9 + k] = p->dt[3 * (size_t)e + k];
    }
    // Jacobians of fixed sides are never written or read; zero the arena once per call so that nothing depends on its history
    OSH_HIP(hipMemsetAsync(base, 0, bytes, s));
    auto up = [&](void* d, const void* h, size_t b) -> int { if (b) OSH_HIP(hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, s)); return OSH_OK; };
    OSH_TRY(up(d_st[0], st.data(), st.size() * 8));
    OSH_TRY(up(d_cst, cst.data(), cst.size() * 8));
    OSH_TRY(up(d_meas, meas.data(), meas.size() * 8));
    OSH_TRY(up(d_eij, p->edge_ij, (size_t)P.E * 8));
    OSH_TRY(up(d_sys, P.sys.data(), n * 4));
    OSH_TRY(up(d_blk_a, P.blk_a.data(), (size_t)P.nblk * 4));
    OSH_TRY(up(d_blk_b, P.blk_b.data(), (size_t)P.nblk * 4));
    OSH_TRY(up(d_ent_ptr, P.ent_ptr.data(), (size_t)(P.nblk + 1) * 4));
    OSH_TRY(up(d_ent, P.ent.data(), P.ent.size() * 4));
    OSH_TRY(up(d_toff, P.toff.data(), NT * 4));
    OSH_TRY(up(d_ttop, P.ttop.data(), NT * 4));
    OSH_TRY(up(d_act_ptr, P.act_ptr.data(), (NT + 1) * 4));
    OSH_TRY(up(d_act, P.act.data(), P.act.size() * 4));
    // the host vectors go out of scope: wait for the copies
    OSH_HIP(hipStreamSynchronize(s));
    return OSH_OK;
  }

  Pgo4View view(int cur) const {
    Pgo4View v;
    v.st = d_st[cur]; v.cst = d_cst; v.eij = d_eij; v.meas = d_meas; v.sys = d_sys; v.J = d_J; v.err = d_err; v.chi = d_chi;
    v.info = info; v.E = P.E;
    return v;
  }
  Asm4View asm_view() const {
    Asm4View a;
    a.J = d_J; a.err = d_err; a.blk_a = d_blk_a; a.blk_b = d_blk_b; a.ent_ptr = d_ent_ptr; a.ent = d_ent; a.H = d_H; a.b = d_b;
    a.info = info; a.nblk = P.nblk;
    return a;
  }
  Env env() const {
    Env g;
    g.T = B->tiles.as<double>(); g.toff = d_toff; g.ttop = d_ttop; g.act_ptr = d_act_ptr; g.act = d_act; g.V = B->V.as<double>();
    g.w = d_w; g.z = d_z; g.fail = d_fail; g.NT = P.NT;
    return g;
  }

  int errors(int cur, int linearize) {
    if (P.E > 0) hipLaunchKernelGGL(k_pgo4_lin, dim3((unsigned)((P.E + 63) / 64)), dim3(64), 0, s, view(cur), linearize);
    return launch_check("k_pgo4_lin");
  }
  int assemble() {
    if (P.nblk > 0) hipLaunchKernelGGL(k_pgo4_assemble, dim3((unsigned)P.nblk), dim3(64), 0, s, asm_view());
    return launch_check("k_pgo4_assemble");
  }
  int max_diag(double* out) {
    hipLaunchKernelGGL(k_pgo4_maxdiag, dim3(1), dim3(256), 0, s, d_H, P.nf, d_red + 4);
    OSH_TRY(launch_check("k_pgo4_maxdiag"));
    OSH_HIP(hipMemcpyAsync(h_red, d_red + 4, 8, hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
    *out = h_red[0];
    return OSH_OK;
  }
  // one trial: (H + lambda I) x = b into d_w, d_st[1 - cur] = UpdateW(d_st[cur], x); chi2 and the scale into h_red
  int trial(int cur, double lambda) {
    const Env g = env();
    OSH_HIP(hipMemsetAsync(d_fail, 0, 4, s));
    OSH_HIP(hipMemsetAsync(B->tiles.p, 0, (size_t)P.ntiles * kTT * 8, s));
    hipLaunchKernelGGL(k_pgo4_fill, dim3((unsigned)P.nblk + 1), dim3(64), 0, s, asm_view(), g, lambda, P.nf);
    OSH_TRY(launch_check("k_pgo4_fill"));
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
    hipLaunchKernelGGL(k_pgo4_step, dim3((unsigned)((P.n + 63) / 64)), dim3(64), 0, s, d_st[cur], d_st[1 - cur], d_cst, d_sys, d_w, d_fail, P.n);
    OSH_TRY(launch_check("k_pgo4_step"));
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

extern "C" int osh_pgo4_solve(osh_lba_ctx* ctx, const osh_pgo4_problem* p, osh_pgo4_result* res) {
  if (!ctx || !res || !res->Rcw || !res->tcw) { set_error("osh_pgo4_solve: bad arguments"); return OSH_ERR_INVALID; }
  Run4 R;
  R.ctx = ctx;
  OSH_TRY(R.check(p));   // refusals leave the result untouched
  res->status = OSH_ERR_DEVICE;
  OSH_TRY(R.setup(p));
  res->envelope_entries = R.P.env_entries;
  res->envelope_tiles = R.P.ntiles;
  res->tall_columns = R.P.tall;
  // SparseOptimizer::optimize (sparse_optimizer.cpp:354-419) with OptimizationAlgorithmLevenberg::solve (levenberg.cpp:99-169)
  int cur = 0, iterations = 0, trials = 0, nBad = 0;
  double lambda = p->lambda_init, ni = 2.0, chi2_initial = 0.0, lambda_used = 0.0;
  const int maxTrials = 10;
  bool ok = true;
  for (int it = 0; it < p->iterations && ok; ++it) {
    OSH_TRY(R.errors(cur, 1));
    double currentChi = 0;
    OSH_TRY(R.chi2_now(&currentChi));
    if (it == 0) chi2_initial = currentChi;
    const double iniChi = currentChi;
    OSH_TRY(R.assemble());
    if (it == 0) {   // computeLambdaInit: the user's value, else tau * max diag(H), tau = 1e-5
      if (p->lambda_init > 0) {
        lambda = p->lambda_init;
      } else {
        double maxd = 0;
        OSH_TRY(R.max_diag(&maxd));
        lambda = 1e-5 * maxd;
      }
      lambda_used = lambda;
      ni = 2;
      nBad = 0;
    }
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
        cur = 1 - cur;   // discardTop: the trial's states become the vertices
      } else {
        lambda *= ni;
        ni *= 2;         // pop: the trial's states are dropped
      }
      ++qmax;
      ++trials;
    } while (rho < 0 && qmax < maxTrials);
    ++iterations;
    if (qmax == maxTrials || rho == 0) { ok = false; continue; }
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;   // the stop rule of this g2o copy (levenberg.cpp:154-164)
    if (nBad >= 3) ok = false;
  }
  OSH_TRY(R.errors(cur, 0));
  double chi2_final = 0;
  OSH_TRY(R.chi2_now(&chi2_final));
  const size_t n = p->n_vertices;
  std::vector<double> st(n * kStateDoubles);
  OSH_HIP(hipMemcpyAsync(st.data(), R.d_st[cur], st.size() * 8, hipMemcpyDeviceToHost, R.s));
  OSH_HIP(hipStreamSynchronize(R.s));
  for (size_t v = 0; v < n; ++v) {
    const double* o = st.data() + v * kStateDoubles;
    for (int k = 0; k < 9; ++k) res->Rcw[9 * v + k] = o[21 + k];
    for (int k = 0; k < 3; ++k) res->tcw[3 * v + k] = o[30 + k];
    if (res->Rwb) for (int k = 0; k < 9; ++k) res->Rwb[9 * v + k] = o[9 + k];
    if (res->twb) for (int k = 0; k < 3; ++k) res->twb[3 * v + k] = o[18 + k];
  }
  res->iterations = iterations;
  res->trials = trials;
  res->chi2_initial = chi2_initial;
  res->chi2_final = chi2_final;
  res->lambda_init_used = lambda_used;
  res->status = OSH_OK;
  return OSH_OK;
}

extern "C" int osh_pgo4_linearize(osh_lba_ctx* ctx, const osh_pgo4_problem* p, double* H, double* b, double* chi2) {
  if (!ctx || !H || !b || !chi2) { set_error("osh_pgo4_linearize: bad arguments"); return OSH_ERR_INVALID; }
  Run4 R;
  R.ctx = ctx;
  OSH_TRY(R.check(p));
  if (R.P.nf > 512) { set_error("osh_pgo4_linearize: %d free vertices, the diagnostic takes up to 512", R.P.nf); return OSH_ERR_UNSUPPORTED; }
  OSH_TRY(R.setup(p));
  OSH_TRY(R.errors(0, 1));
  OSH_TRY(R.chi2_now(chi2));
  OSH_TRY(R.assemble());
  std::vector<double> blocks((size_t)R.P.nblk * 16);
  if (!blocks.empty()) OSH_HIP(hipMemcpyAsync(blocks.data(), R.d_H, blocks.size() * 8, hipMemcpyDeviceToHost, R.s));
  if (R.P.N > 0) OSH_HIP(hipMemcpyAsync(b, R.d_b, (size_t)R.P.N * 8, hipMemcpyDeviceToHost, R.s));
  OSH_HIP(hipStreamSynchronize(R.s));
  const size_t N = R.P.N;
  std::fill(H, H + N * N, 0.0);
  for (int k = 0; k < R.P.nblk; ++k) {
    const int a = R.P.blk_a[k], bb = R.P.blk_b[k];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        const double h = blocks[(size_t)k * 16 + r * 4 + c];
        H[(size_t)(4 * a + r) * N + 4 * bb + c] = h;
        if (a != bb) H[(size_t)(4 * bb + c) * N + 4 * a + r] = h;
      }
  }
  return OSH_OK;
}
