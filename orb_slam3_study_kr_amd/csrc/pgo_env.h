// pgo_env.h -- the parts of the pose-graph solvers that do not depend on the vertex type, shared by pgo_device.hip (Sim3,
// 7 unknowns per vertex) and pgo4_device.hip (4-DoF, 4 unknowns per vertex): the envelope LDL^T kernels, the fixed-order
// chi2 / computeScale reduction, and the host-side plan (free-vertex numbering, the assembly CSR of dim x dim blocks, the
// envelope and the active lists of every panel).  The LDL^T works on scalar unknowns: only the plan knows `dim`.
//
// Envelope storage: the reduced system has dim nf unknowns (free vertices in array order = keyframe-id order), padded to a
// multiple of 32 with an identity diagonal.  Column tile J keeps row tiles ttop[J] .. J (32 x 32 doubles each, row-major),
// where ttop[J] is the row tile of the first non-zero of any column in J.  LDL^T creates no fill above a column's first
// non-zero, so the factor lives in the same tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>
#include "common.h"
#include "ldlt_block.h"

// No FMA contraction, as in the vertex algebra: the factorisation and the reductions round every operation, so that both graphs
// solve in the same bits whichever header a translation unit includes first.
#pragma clang fp contract(off)

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

struct PgoBuffers {
  DevBuf arena, tiles, V;
  PinBuf h_red;
};

int launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("kernel launch %s failed: %s", what, hipGetErrorString(e)); return OSH_ERR_DEVICE; }
  return OSH_OK;
}

}  // namespace
}  // namespace osh
