// pgo_env.h -- the parts of the pose-graph solvers that do not depend on the vertex type, shared by pgo_device.hip (Sim3,
// 7 unknowns per vertex) and pgo4_device.hip (4-DoF, 4 unknowns per vertex): the envelope LDL^T kernels, the fixed-order
// chi2 / computeScale reduction, the host-side plan (free-vertex numbering, the assembly CSR of dim x dim blocks, the
// envelope and the active lists of every panel), k_pgo_fill, k_pgo_maxdiag, and PgoRun: the arena, the trial sequence, g2o's
// Levenberg loop and the dense diagnostic.  The LDL^T works on scalar unknowns: only the plan knows `dim`.
//
// Envelope storage: the reduced system has dim nf unknowns (free vertices in array order = keyframe-id order), padded to a
// multiple of 32 with an identity diagonal.  Column tile J keeps row tiles ttop[J] .. J (32 x 32 doubles each, row-major),
// where ttop[J] is the row tile of the first non-zero of any column in J.  LDL^T creates no fill above a column's first
// non-zero, so the factor lives in the same tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <type_traits>
#include <vector>
#include "common.h"
#include "ldlt_block.h"

// No FMA contraction, as in the vertex algebra: the factorisation and the reductions round every operation, so that both graphs
// solve in the same bits whichever header a translation unit includes first.
#pragma clang fp contract(off)
#include "g2o_lm.h"   // below the pragma: PgoRun::solve's controller is compiled without contraction in both graphs, as it was

namespace osh {
namespace {

constexpr int kT = 32;            // tile edge = panel width
constexpr int kTT = kT * kT;

struct Env {
  double* T;            // tiles
  const int* toff;      // [NT] first tile of column tile J
  const int* ttop;      // [NT]
  const int* act_ptr;   // [NT + 1]
  const int* act;       // active column tiles of every panel (ascending)
  double* V;            // [max active][32][32] unscaled panel rows D1 U12
  double* w;            // [32 NT] rhs -> solution
  double* z;            // [32 NT] unscaled forward-substituted rhs
  int* fail;
  int NT;
};

__device__ __forceinline__ double* env_tile(const Env& g, int I, int J) { return g.T + (size_t)(g.toff[J] + I - g.ttop[J]) * kTT; }

// one wavefront factors diagonal tile p in registers (lane j keeps column j) and forward-substitutes the panel's rhs
__global__ __launch_bounds__(64) void k_env_diag(Env g, int p) {
  if (*g.fail) return;
  double* D = env_tile(g, p, p);
  const int lane = threadIdx.x;
  const int j = lane < kT ? lane : 0;
  double col[kT];
#pragma unroll
  for (int r = 0; r < kT; ++r) col[r] = r <= j ? D[r * kT + j] : (r == j ? 1.0 : 0.0);
  double zr = lane < kT ? g.w[kT * p + lane] : 0.0;
  bool zero_pivot = false;
#pragma unroll
  for (int k = 0; k < kT; ++k) {
    const double d = ldlt_readlane(col[k], k);
    zero_pivot |= (d == 0.0);
    const double lk = col[k] / d;
    const double zk = ldlt_readlane(zr, k);
    if (lane > k) zr -= lk * zk;
#pragma unroll
    for (int i = k + 1; i < kT; ++i) col[i] -= ldlt_readlane(lk, i) * col[k];
  }
  if (zero_pivot) { if (lane == 0) *g.fail = 1; return; }
  double dd[kT];
#pragma unroll
  for (int r = 0; r < kT; ++r) dd[r] = ldlt_readlane(col[r], r);
  if (lane < kT) {
    double dl = 1.0;
#pragma unroll
    for (int r = 0; r < kT; ++r) {
      if (r <= lane) D[r * kT + lane] = (r == lane) ? dd[r] : col[r] / dd[r];
      if (r == lane) dl = dd[r];
    }
    g.z[kT * p + lane] = zr;
    g.w[kT * p + lane] = zr / dl;
  }
}

// block per active column tile of panel p, thread per column: V12 = U11^-T A12, U12 = D1^-1 V12, rhs b2 -= U12^T z1
__global__ __launch_bounds__(64) void k_env_panel(Env g, int p) {
  if (*g.fail) return;
  __shared__ double U11[kT][kT + 1];
  __shared__ double d1[kT], z1[kT];
  const int tid = threadIdx.x;
  const double* D = env_tile(g, p, p);
  for (int idx = tid; idx < kTT; idx += 64) {
    const int r = idx / kT, c = idx - r * kT;
    const double a = D[r * kT + (c >= r ? c : r)];
    if (c == r) d1[r] = a;
    U11[r][c] = c > r ? a : 0.0;
  }
  if (tid < kT) z1[tid] = g.z[kT * p + tid];
  __syncthreads();
  if (tid >= kT) return;
  const int ai = blockIdx.x, J = g.act[g.act_ptr[p] + ai];
  double* Tl = env_tile(g, p, J);
  double* Vo = g.V + (size_t)ai * kTT;
  double v[kT];
#pragma unroll
  for (int r = 0; r < kT; ++r) v[r] = Tl[r * kT + tid];
#pragma unroll
  for (int r = 1; r < kT; ++r) {
    double s = v[r];
#pragma unroll
    for (int k = 0; k < r; ++k) s -= U11[k][r] * v[k];
    v[r] = s;
  }
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < kT; ++r) {
    const double u = v[r] / d1[r];
    Vo[r * kT + tid] = v[r];
    Tl[r * kT + tid] = u;
    acc += u * z1[r];
  }
  g.w[kT * J + tid] -= acc;
}

// tile (Ja, Jb), Ja <= Jb both active in panel p: A(Ja, Jb) -= U(p, Ja)^T V(p, Jb), 2 x 2 MFMA 16x16x4 outputs, K = 32.
// Operand layout: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[row = (lane >> 4) + 4 reg][col = lane & 15].
__global__ __launch_bounds__(64) void k_env_update(Env g, int p) {
  const int x = blockIdx.x, y = blockIdx.y;
  if (x > y || *g.fail) return;
  typedef double f64x4 __attribute__((ext_vector_type(4)));
  __shared__ double Us[kT][kT + 4], Vs[kT][kT + 4];
  const int ap = g.act_ptr[p];
  const int Ja = g.act[ap + x], Jb = g.act[ap + y];
  const double* U = env_tile(g, p, Ja);
  const double* V = g.V + (size_t)y * kTT;
  const int lane = threadIdx.x;
  for (int idx = lane; idx < kTT; idx += 64) {
    const int r = idx / kT, c = idx - r * kT;
    Us[r][c] = U[idx];
    Vs[r][c] = V[idx];
  }
  __syncthreads();
  double* O = env_tile(g, Ja, Jb);
  const int lrow = lane >> 4, lcol = lane & 15;
#pragma unroll
  for (int si = 0; si < 2; ++si) {
    double a[kT / 4];
#pragma unroll
    for (int q = 0; q < kT / 4; ++q) a[q] = Us[4 * q + lrow][16 * si + lcol];
#pragma unroll
    for (int sj = 0; sj < 2; ++sj) {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < kT / 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], Vs[4 * q + lrow][16 * sj + lcol], acc, 0, 0, 0);
      const int col = 16 * sj + lcol;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 16 * si + lrow + 4 * reg;
        if (x != y || col >= row) O[row * kT + col] -= acc[reg];
      }
    }
  }
}

// x = U^-1 w, panels in reverse: s_r = sum over the panel's active tiles of u_rj x_j (two rows per wavefront, fixed order),
// then the 32x32 unit upper triangle of the diagonal tile
__global__ __launch_bounds__(1024) void k_env_back(Env g) {
  if (*g.fail) return;
  __shared__ double U11[kT][kT + 1];
  __shared__ double srow[kT];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  for (int p = g.NT - 1; p >= 0; --p) {
    const double* D = env_tile(g, p, p);
    for (int idx = tid; idx < kTT; idx += 1024) {
      const int r = idx / kT, c = idx - r * kT;
      U11[r][c] = c > r ? D[idx] : 0.0;
    }
    const int a0 = g.act_ptr[p], na = g.act_ptr[p + 1] - a0;
    for (int r = wv; r < kT; r += 16) {
      double s = 0.0;
      for (int idx = lane; idx < na * kT; idx += 64) {
        const int J = g.act[a0 + idx / kT], c = idx & (kT - 1);
        s += env_tile(g, p, J)[r * kT + c] * g.w[kT * J + c];
      }
      s = dev::wave_sum(s);
      if (lane == 0) srow[r] = s;
    }
    __syncthreads();
    if (wv == 0) {
      double t = lane < kT ? g.w[kT * p + lane] - srow[lane] : 0.0;
#pragma unroll
      for (int c = kT - 1; c > 0; --c) {
        const double xc = ldlt_readlane(t, c);
        if (lane < c) t -= U11[lane < kT ? lane : 0][c] * xc;
      }
      if (lane < kT) g.w[kT * p + lane] = t;
    }
    __threadfence_block();
    __syncthreads();
  }
}

// out[0] = sum of the edges' chi2, out[1] = computeScale = sum x (lambda x + b) (levenberg.cpp:187-194), both in a fixed order
__global__ __launch_bounds__(1024) void k_pgo_reduce(const double* chi, int E, const double* x, const double* b, int N, double lambda,
                                                     int with_scale, double* out) {
  __shared__ double red[2][1024];
  const int t = threadIdx.x;
  double c = 0, s = 0;
  for (int e = t; e < E; e += 1024) c += chi[e];
  if (with_scale) for (int k = t; k < N; k += 1024) s += x[k] * (lambda * x[k] + b[k]);
  red[0][t] = c; red[1][t] = s;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if (t < h) { red[0][t] += red[0][t + h]; red[1][t] += red[1][t + h]; }
    __syncthreads();
  }
  if (t == 0) { out[0] = red[0][0]; out[1] = red[1][0]; }
}

// Host-side structure of one graph: free-vertex numbering, assembly CSR, envelope and active lists.
struct PlanInput {
  int n_vertices, n_edges, solve_mode;
  const uint8_t* fixed;
  const int32_t* edge_ij;
};

struct Plan {
  int n = 0, nf = 0, E = 0, N = 0, NT = 0, ntiles = 0, nblk = 0, max_act = 0, tall = 0;
  int64_t env_entries = 0;
  std::vector<int> sys, blk_a, blk_b, ent_ptr, ent, toff, ttop, act_ptr, act;
};

// `dim` unknowns per free vertex; `tag` prefixes the error messages.
int make_plan(const PlanInput& p, int dim, const char* tag, Plan& P) {
  P.n = p.n_vertices; P.E = p.n_edges;
  P.sys.assign(P.n, -1);
  for (int v = 0; v < P.n; ++v) if (!p.fixed[v]) P.sys[v] = P.nf++;
  if (P.nf > OSH_PGO_MAX_VERTICES) {
    set_error("%s: %d free vertices, the limit is %d", tag, P.nf, OSH_PGO_MAX_VERTICES);
    return OSH_ERR_UNSUPPORTED;
  }
  for (int e = 0; e < P.E; ++e) {
    const int i = p.edge_ij[2 * e], j = p.edge_ij[2 * e + 1];
    if (i < 0 || j < 0 || i >= P.n || j >= P.n || i == j) { set_error("%s: edge %d joins vertices %d and %d", tag, e, i, j); return OSH_ERR_INVALID; }
  }
  // diagonal blocks first (free vertex order), then the off-diagonal pairs in (a, b) order; entries in edge order
  std::vector<std::vector<int>> diag(P.nf);
  std::map<std::pair<int, int>, std::vector<int>> off;
  std::vector<int> minnb(P.nf);
  for (int a = 0; a < P.nf; ++a) minnb[a] = a;
  for (int e = 0; e < P.E; ++e) {
    const int si = P.sys[p.edge_ij[2 * e]], sj = P.sys[p.edge_ij[2 * e + 1]];
    if (si >= 0) diag[si].push_back(e << 1);
    if (sj >= 0) diag[sj].push_back(e << 1 | 1);
    if (si >= 0 && sj >= 0 && si != sj) {
      const int a = std::min(si, sj), b = std::max(si, sj);
      off[{a, b}].push_back(e << 1 | (si == a ? 0 : 1));
      minnb[b] = std::min(minnb[b], a);
    }
  }
  P.ent_ptr.assign(1, 0);
  for (int a = 0; a < P.nf; ++a) {
    P.blk_a.push_back(a); P.blk_b.push_back(a);
    P.ent.insert(P.ent.end(), diag[a].begin(), diag[a].end());
    P.ent_ptr.push_back((int)P.ent.size());
  }
  for (const auto& kv : off) {
    P.blk_a.push_back(kv.first.first); P.blk_b.push_back(kv.first.second);
    P.ent.insert(P.ent.end(), kv.second.begin(), kv.second.end());
    P.ent_ptr.push_back((int)P.ent.size());
  }
  P.nblk = (int)P.blk_a.size();
  P.N = dim * P.nf;
  P.NT = std::max(1, (P.N + kT - 1) / kT);
  P.ttop.assign(P.NT, 0);
  P.env_entries = 0; P.tall = 0;
  for (int a = 0; a < P.nf; ++a) {
    P.env_entries += dim * (int64_t)(dim * (a - minnb[a])) + dim * (dim + 1) / 2;
    if (dim * (a - minnb[a]) > 64) ++P.tall;
  }
  for (int J = 0; J < P.NT; ++J) {
    int top = J;
    if (p.solve_mode != OSH_PGO_SOLVE_DENSE) {
      for (int c = kT * J; c < std::min(P.N, kT * J + kT); ++c) top = std::min(top, (dim * minnb[c / dim]) / kT);
    } else {
      top = 0;
    }
    P.ttop[J] = top;
  }
  P.toff.assign(P.NT, 0);
  int64_t tiles = 0;
  for (int J = 0; J < P.NT; ++J) { P.toff[J] = (int)std::min<int64_t>(tiles, INT32_MAX); tiles += J - P.ttop[J] + 1; }
  if (tiles > OSH_PGO_MAX_ENV_TILES) {
    set_error("%s: the envelope needs %lld tiles of 32x32, the limit is %d", tag, (long long)tiles, OSH_PGO_MAX_ENV_TILES);
    return OSH_ERR_UNSUPPORTED;
  }
  P.ntiles = (int)tiles;
  std::vector<std::vector<int>> lists(P.NT);
  for (int J = 0; J < P.NT; ++J) for (int q = P.ttop[J]; q < J; ++q) lists[q].push_back(J);
  P.act_ptr.assign(1, 0);
  P.max_act = 1;
  for (int q = 0; q < P.NT; ++q) {
    P.act.insert(P.act.end(), lists[q].begin(), lists[q].end());
    P.act_ptr.push_back((int)P.act.size());
    P.max_act = std::max(P.max_act, (int)lists[q].size());
  }
  if (P.act.empty()) P.act.push_back(0);
  return OSH_OK;
}

// The arrays k_pgo_assemble and k_pgo_fill read.  A graph's assembly view derives from it and adds nblk (after its information,
// if it has one).
struct AsmArrays {
  const double* J; const double* err;
  const int* blk_a; const int* blk_b;     // [nblk] free-vertex indices (a == b: diagonal block), a <= b
  const int* ent_ptr; const int* ent;     // [nblk + 1], entries: diagonal (e << 1 | side), off-diagonal (e << 1 | flip)
  double* H;                              // [nblk][D D]
  double* b;                              // [D nf]
};

// block per D x D block of H: sums its edges in edge order (CSR built at upload, no atomics); b = -J^T Omega e.  Each edge side
// has an M x D Jacobian (row-major); Omega is the identity, or the diagonal v.info.w when kDiagInfo.
template <int D, int M, bool kDiagInfo, class AsmV>
__global__ __launch_bounds__(64) void k_pgo_assemble(AsmV v) {
  const int k = blockIdx.x, t = threadIdx.x;
  const int a = v.blk_a[k], bb = v.blk_b[k];
  const int p0 = v.ent_ptr[k], p1 = v.ent_ptr[k + 1];
  auto omega = [&](double j, int m) {
    if constexpr (kDiagInfo) return j * v.info.w[m]; else return j;
  };
  if (t < D * D) {
    const int r = t / D, c = t - D * (t / D);
    double s = 0;
    for (int q = p0; q < p1; ++q) {
      const int en = v.ent[q], e = en >> 1, f = en & 1;
      const double* Ja = v.J + ((size_t)e * 2 + f) * (M * D);
      const double* Jb = a == bb ? Ja : v.J + ((size_t)e * 2 + (1 - f)) * (M * D);
      double h = 0;
      for (int m = 0; m < M; ++m) h += omega(Ja[m * D + r], m) * Jb[m * D + c];
      s += h;
    }
    v.H[(size_t)k * (D * D) + t] = s;
  } else if (a == bb && t < D * D + D) {
    const int r = t - D * D;
    double s = 0;
    for (int q = p0; q < p1; ++q) {
      const int en = v.ent[q], e = en >> 1, f = en & 1;
      const double* Ja = v.J + ((size_t)e * 2 + f) * (M * D);
      const double* er = v.err + M * (size_t)e;
      double h = 0;
      for (int m = 0; m < M; ++m) h += omega(Ja[m * D + r], m) * er[m];
      s -= h;
    }
    v.b[D * a + r] = s;
  }
}

// H + lambda I into the envelope tiles of the working matrix, b into the right-hand side.  D unknowns per vertex; `v` is the
// graph's assembly view (blk_a, blk_b, H of D x D blocks, b, nblk).
template <int D, class AsmV>
__global__ __launch_bounds__(64) void k_pgo_fill(AsmV v, Env g, double lambda, int nf) {
  const int k = blockIdx.x, t = threadIdx.x;
  if (k == v.nblk) {   // padding of the last tile: identity, zero rhs
    for (int R = D * nf + t; R < kT * g.NT; R += 64) { env_tile(g, R >> 5, R >> 5)[(R & 31) * kT + (R & 31)] = 1.0; g.w[R] = 0.0; }
    return;
  }
  const int a = v.blk_a[k], bb = v.blk_b[k];
  if (t < D * D) {
    const int r = t / D, c = t - D * (t / D);
    const int R = D * a + r, Cc = D * bb + c;
    if (R <= Cc) {
      double h = v.H[(size_t)k * (D * D) + t];
      if (R == Cc) h += lambda;
      env_tile(g, R >> 5, Cc >> 5)[(R & 31) * kT + (Cc & 31)] = h;
    }
  } else if (a == bb && t < D * D + D) {
    g.w[D * a + t - D * D] = v.b[D * a + t - D * D];
  }
}

// max |H_kk| over the diagonal blocks 0 .. nf-1 (they come first in the block list); max is exact in any order
template <int D>
__global__ __launch_bounds__(256) void k_pgo_maxdiag(const double* H, int nf, double* out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double m = 0.0;
  for (int k = t; k < D * nf; k += 256) m = fmax(m, fabs(H[(size_t)(k / D) * (D * D) + (k % D) * (D + 1)]));
  red[t] = m;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] = fmax(red[t], red[t + h]);
    __syncthreads();
  }
  if (t == 0) *out = red[0];
}

struct PgoBuffers {
  DevBuf arena, tiles, V;
  PinBuf h_red;
};

struct LmResult {
  int iterations = 0, trials = 0, cur = 0;   // the returned states are d_x[cur]
  double chi2_initial = 0, chi2_final = 0, lambda0 = 0;
};

// Everything of one call on the device for the graph G: the arena, the upload, one LM trial, the LM loop and the dense
// diagnostic.  G gives
//   D, M               unknowns per vertex, errors per edge
//   kState, kMeas      doubles of one vertex state and of one edge measurement
//   Aux, kAux          its per-vertex device array (type, entries per vertex)
//   kDiagInfo, kTag    k_pgo_assemble's information (identity or diagonal), the prefix of its messages
//   lin(R, cur, linearize), step(R, cur)   its kernel launches, each returning launch_check's result
//   asm_view(R)        the view k_pgo_assemble and k_pgo_fill read
template <class G>
struct PgoRun {
  osh_lba_ctx* ctx;
  G graph;
  hipStream_t s = nullptr;
  PgoBuffers* B = nullptr;
  Plan P;
  double *d_x[2] = {nullptr, nullptr}, *d_meas, *d_J, *d_err, *d_chi, *d_H, *d_b, *d_w, *d_z, *d_red;
  int *d_eij, *d_sys, *d_blk_a, *d_blk_b, *d_ent_ptr, *d_ent, *d_toff, *d_ttop, *d_act_ptr, *d_act, *d_fail;
  typename G::Aux* d_aux;
  double* h_red = nullptr;

  explicit PgoRun(osh_lba_ctx* c) : ctx(c) {}

  // the size checks: no device work
  int plan(const PlanInput& in) { return make_plan(in, G::D, G::kTag, P); }
  int dense_fits() const {
    if (P.nf > 512) { set_error("%s_linearize: %d free vertices, the diagnostic takes up to 512", G::kTag, P.nf); return OSH_ERR_UNSUPPORTED; }
    return OSH_OK;
  }

  // the arena (zeroed), the plan, the initial states x0 into d_x[0], the measurements, the edges and the per-vertex array
  int upload(const double* x0, const double* meas, const int32_t* eij, const typename G::Aux* aux) {
    int device = 0;
    OSH_TRY(lba_stream(ctx, &device, &s));
    B = attachment<PgoBuffers>(ctx, kAttachPgo);
    if (!B) return OSH_ERR_INVALID;
    const size_t n = P.n, E = std::max(P.E, 1), NT = P.NT;
    Layout L;
    const auto s_x0 = L.take<double>(n * G::kState), s_x1 = L.take<double>(n * G::kState);
    const auto s_aux = L.take<typename G::Aux>(n * G::kAux);
    const auto s_meas = L.take<double>(E * G::kMeas), s_J = L.take<double>(E * 2 * G::D * G::M), s_err = L.take<double>(E * G::M), s_chi = L.take<double>(E),
               s_H = L.take<double>((size_t)P.nblk * G::D * G::D), s_b = L.take<double>((size_t)P.N + 1), s_w = L.take<double>(NT * kT),
               s_z = L.take<double>(NT * kT), s_red = L.take<double>(8);
    const auto s_eij = L.take<int>(E * 2), s_sys = L.take<int>(n), s_blk_a = L.take<int>(P.nblk), s_blk_b = L.take<int>(P.nblk), s_ent_ptr = L.take<int>(P.nblk + 1),
               s_ent = L.take<int>(P.ent.size() + 1), s_toff = L.take<int>(NT), s_ttop = L.take<int>(NT), s_act_ptr = L.take<int>(NT + 1),
               s_act = L.take<int>(P.act.size()), s_fail = L.take<int>(1);
    OSH_TRY(B->arena.reserve(L.bytes));
    OSH_TRY(B->tiles.reserve((size_t)P.ntiles * kTT * 8));
    OSH_TRY(B->V.reserve((size_t)P.max_act * kTT * 8));
    h_red = static_cast<double*>(B->h_red.reserve(64));
    if (!h_red) { set_error("%s: pinned allocation failed", G::kTag); return OSH_ERR_DEVICE; }
    char* const a = B->arena.as<char>();
    d_x[0] = s_x0.in(a); d_x[1] = s_x1.in(a); d_aux = s_aux.in(a); d_meas = s_meas.in(a); d_J = s_J.in(a); d_err = s_err.in(a); d_chi = s_chi.in(a);
    d_H = s_H.in(a); d_b = s_b.in(a); d_w = s_w.in(a); d_z = s_z.in(a); d_red = s_red.in(a); d_eij = s_eij.in(a); d_sys = s_sys.in(a);
    d_blk_a = s_blk_a.in(a); d_blk_b = s_blk_b.in(a); d_ent_ptr = s_ent_ptr.in(a); d_ent = s_ent.in(a); d_toff = s_toff.in(a); d_ttop = s_ttop.in(a);
    d_act_ptr = s_act_ptr.in(a); d_act = s_act.in(a); d_fail = s_fail.in(a);
    // Jacobians of fixed sides are never written or read; zero the arena once per call so that nothing depends on its history
    OSH_HIP(hipMemsetAsync(B->arena.p, 0, L.bytes, s));
    auto up = [&](void* d, const void* h, size_t b) -> int { if (b) OSH_HIP(hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, s)); return OSH_OK; };
    OSH_TRY(up(d_x[0], x0, n * G::kState * 8));
    OSH_TRY(up(d_aux, aux, n * G::kAux * sizeof(typename G::Aux)));
    OSH_TRY(up(d_meas, meas, (size_t)P.E * G::kMeas * 8));
    OSH_TRY(up(d_eij, eij, (size_t)P.E * 8));
    OSH_TRY(up(d_sys, P.sys.data(), n * 4));
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

  Env env() const {
    Env g;
    g.T = B->tiles.as<double>(); g.toff = d_toff; g.ttop = d_ttop; g.act_ptr = d_act_ptr; g.act = d_act; g.V = B->V.as<double>();
    g.w = d_w; g.z = d_z; g.fail = d_fail; g.NT = P.NT;
    return g;
  }

  AsmArrays asm_arrays() const { return AsmArrays{d_J, d_err, d_blk_a, d_blk_b, d_ent_ptr, d_ent, d_H, d_b}; }

  // errors (and Jacobians) at d_x[cur]
  int errors(int cur, int linearize) { return graph.lin(*this, cur, linearize); }
  int assemble() {
    if (P.nblk > 0) hipLaunchKernelGGL((k_pgo_assemble<G::D, G::M, G::kDiagInfo>), dim3((unsigned)P.nblk), dim3(64), 0, s, graph.asm_view(*this));
    return launch_check("k_pgo_assemble");
  }
  int max_diag(double* out) {
    hipLaunchKernelGGL(k_pgo_maxdiag<G::D>, dim3(1), dim3(256), 0, s, d_H, P.nf, d_red + 4);
    OSH_TRY(launch_check("k_pgo_maxdiag"));
    OSH_HIP(hipMemcpyAsync(h_red, d_red + 4, 8, hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
    *out = h_red[0];
    return OSH_OK;
  }
  // one trial: (H + lambda I) x = b into d_w, d_x[1 - cur] = x (+) d_x[cur]; chi2, the scale and the fail flag into h_red
  int trial(int cur, double lambda) {
    const Env g = env();
    OSH_HIP(hipMemsetAsync(d_fail, 0, 4, s));
    OSH_HIP(hipMemsetAsync(B->tiles.p, 0, (size_t)P.ntiles * kTT * 8, s));
    hipLaunchKernelGGL(k_pgo_fill<G::D>, dim3((unsigned)P.nblk + 1), dim3(64), 0, s, graph.asm_view(*this), g, lambda, P.nf);
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
    OSH_TRY(graph.step(*this, cur));
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

  // SparseOptimizer::optimize (sparse_optimizer.cpp:354-419) with OptimizationAlgorithmLevenberg::solve (levenberg.cpp:99-169).
  // lambda0(&l) is computeLambdaInit, called once after the first assembly.
  template <class Lambda0>
  int solve(int max_iterations, Lambda0 lambda0, LmResult& out) {
    int cur = 0, nBad = 0;
    double lambda = 0.0, ni = 2.0;
    bool ok = true;
    for (int it = 0; it < max_iterations && ok; ++it) {
      OSH_TRY(errors(cur, 1));
      double currentChi = 0;
      OSH_TRY(chi2_now(&currentChi));
      if (it == 0) out.chi2_initial = currentChi;
      const double iniChi = currentChi;
      OSH_TRY(assemble());
      if (it == 0) {
        OSH_TRY(lambda0(&lambda));
        out.lambda0 = lambda;
        ni = 2;
        nBad = 0;
      }
      double rho = 0;
      int qmax = 0;
      do {
        OSH_TRY(trial(cur, lambda));
        double tempChi = h_red[0];
        int fail = 0;
        std::memcpy(&fail, &h_red[2], 4);
        if (fail) tempChi = std::numeric_limits<double>::max();
        const LmTrial t = lm_judge_trial(lambda, ni, currentChi, tempChi, h_red[1]);
        rho = t.rho;
        if (t.accepted) {
          currentChi = tempChi;
          cur = 1 - cur;   // discardTop: the trial's states become the vertices (pop: a rejected trial's states are dropped)
        }
        ++qmax;
        ++out.trials;
      } while (rho < 0 && qmax < kLmMaxTrials);
      ++out.iterations;
      ok = lm_iteration_goes_on(nBad, iniChi, currentChi, qmax, rho);
    }
    // computeActiveErrors at the returned states
    OSH_TRY(errors(cur, 0));
    OSH_TRY(chi2_now(&out.chi2_final));
    out.cur = cur;
    return OSH_OK;
  }

  // the *_linearize diagnostic at the uploaded states: chi2, b, and H expanded from its D x D blocks into dense N x N
  int linearize(double* H, double* b, double* chi2) {
    constexpr int D = G::D;
    OSH_TRY(errors(0, 1));
    OSH_TRY(chi2_now(chi2));
    OSH_TRY(assemble());
    std::vector<double> blocks((size_t)P.nblk * D * D);
    if (!blocks.empty()) OSH_HIP(hipMemcpyAsync(blocks.data(), d_H, blocks.size() * 8, hipMemcpyDeviceToHost, s));
    if (P.N > 0) OSH_HIP(hipMemcpyAsync(b, d_b, (size_t)P.N * 8, hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
    const size_t N = P.N;
    std::fill(H, H + N * N, 0.0);
    for (int k = 0; k < P.nblk; ++k) {
      const int a = P.blk_a[k], bb = P.blk_b[k];
      for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
          const double h = blocks[(size_t)k * D * D + r * D + c];
          H[(size_t)(D * a + r) * N + D * bb + c] = h;
          if (a != bb) H[(size_t)(D * bb + c) * N + D * a + r] = h;
        }
    }
    return OSH_OK;
  }
};

}  // namespace
}  // namespace osh
