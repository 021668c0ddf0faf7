// block_kit.h -- the pieces the one-block-per-problem kernels share (device only): k_pose_opt (pose_device.hip), k_posei
// (posei_device.hip), k_sim3_opt and k_sim3_lin (sim3opt_device.hip).
//
//   upper_index / upper_diag      entries of an upper triangle packed row by row
//   block_sum_n_*<NT, N>          N block sums with two barriers, added in wavefront order
//   upper_max_abs_diag<N>         max |H_dd| of computeLambdaInit
//   ldlt_solve_upper<N>           (H + lambda I) x = b by one thread, fully unrolled
//
// Contraction: this header has no `fp contract` pragma of its own, so every function is compiled under the setting in force
// where the header is included.  sim3opt_device.hip runs without FMA contraction from the point where it includes pgo_sim3.h
// and therefore includes this header after it; pose_device.hip and posei_device.hip use the compiler's default.  A
// translation unit sees one setting only, so the kit never mixes the two.
// Summation order: every sum keeps the order and the parentheses the kernels had before they shared this file (the result bits
// depend on them).
// Not here: the per-edge H += J^T (w Omega) J, b += J^T (-w Omega r).  Where contraction is allowed the compiler is free to
// fuse either product of `p + q` into the addition, and which one it takes follows the order of the surrounding code: with the
// loops of pose_device.hip and posei_device.hip moved into this header their result bits changed, so every file keeps its own
// loop.
#pragma once
#include "lba_math.h"

namespace osh {
namespace dev {

// entry (a, c), a <= c, of the upper triangle of an N x N matrix packed row by row; (k, k) for the diagonal
constexpr int upper_index(int N, int a, int c) { return a * N - a * (a - 1) / 2 + (c - a); }
constexpr int upper_diag(int N, int k) { return upper_index(N, k, k); }

// N block sums of a block of NT threads with TWO barriers: butterfly inside each wavefront, the wavefront partials parked in
// shn[NT / 64][N]; block_sum_total then adds the partials of one value in wavefront order (deterministic).  One barrier pair
// per value cost 54 barriers per iteration of the 6-unknown kernels.
template <int NT, int N>
__device__ __forceinline__ void block_sum_park(double* v, double* shn) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) shn[(threadIdx.x >> 6) * N + k] = v[k];
  }
  __syncthreads();
}
template <int NT, int N>
__device__ __forceinline__ double block_sum_total(const double* shn, int k) {
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) t += shn[w * N + k];
  return t;
}
// every thread ends with all N totals in v
template <int NT, int N>
__device__ __forceinline__ void block_sum_n_all(double* v, double* shn) {
  block_sum_park<NT, N>(v, shn);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = block_sum_total<NT, N>(shn, k);
}
// thread k < N writes total k to out[k] (LDS); the caller's next barrier publishes it
template <int NT, int N>
__device__ __forceinline__ void block_sum_n_to(double* v, double* shn, double* out) {
  block_sum_park<NT, N>(v, shn);
  if (threadIdx.x < N) out[threadIdx.x] = block_sum_total<NT, N>(shn, threadIdx.x);
}

// max |H_dd| over the diagonal of a packed upper triangle (computeLambdaInit, optimization_algorithm_levenberg.cpp:171-185)
template <int N>
__device__ __forceinline__ double upper_max_abs_diag(const double* H) {
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) m = fmax(m, fabs(H[upper_diag(N, k)]));
  return m;
}

// (H + lambda I) x = b by LDL^T on the calling thread, H the packed upper triangle; false unless every pivot is positive
// (LinearSolverDense, linear_solver_dense.h:97-105: Eigen's LDLT and isPositive), and then x = 0.
// Every loop is unrolled: with run-time indices the N x N array lives in scratch memory and this one-thread section was most of
// an iteration.  A non-positive pivot does not leave the loop early; its results are simply not used.
template <int N>
__device__ __forceinline__ bool ldlt_solve_upper(const double* sys_H, const double* sys_b, double lambda, double* x) {
  double A[N * N];
  {
    int m = 0;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
      for (int c = a; c < N; ++c) { A[a * N + c] = sys_H[m] + ((a == c) ? lambda : 0.0); ++m; }
  }
  bool good = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double dk = A[k * N + k];
    good = good && (dk > 0.0);
    double l[N];
#pragma unroll
    for (int i = k + 1; i < N; ++i) l[i] = A[k * N + i] / dk;
#pragma unroll
    for (int i = k + 1; i < N; ++i)
#pragma unroll
      for (int j = i; j < N; ++j) A[i * N + j] -= l[i] * A[k * N + j];
#pragma unroll
    for (int i = k + 1; i < N; ++i) A[k * N + i] = l[i];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = sys_b[k];
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int i = k + 1; i < N; ++i) x[i] -= A[k * N + i] * x[k];
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] /= A[k * N + k];
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    double s = x[k];
#pragma unroll
    for (int i = k + 1; i < N; ++i) s -= A[k * N + i] * x[i];
    x[k] = s;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = good ? x[k] : 0.0;
  return good;
}

}  // namespace dev
}  // namespace osh
