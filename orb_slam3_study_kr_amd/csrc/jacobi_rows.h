// jacobi_rows.h -- the one-sided Jacobi method on FP64 rows that two_view.h (the 16x9 systems of H and F, the 3x3 SVD), mlpnp.h (the
// 12x12 normal matrix, the 3x3 eigenvectors and polar factor) and sim3_ransac.h (the rotation of its two-sided 4x4 method) share.
// Plain C++ and device code alike; every statement is a single IEEE operation with contraction off, no loop depends on the data.
//   * A column pair (p, q) is rotated from alpha = sum a_ip^2, beta = sum a_iq^2, gamma = sum a_ip a_iq; a pair whose columns are
//     orthogonal already (gamma == 0) is not rotated.  A sweep visits the pairs in cyclic order (0,1) (0,2) .. (COLS-2,COLS-1).
//   * For an array of kJacobiRows rows every sum over the rows is the pairwise tree ((r0+r1)+(r2+r3))+.. (tree16): the device keeps
//     one row per lane and adds across the 16 lanes in exactly that tree (rows_sum), so host and device run the same operations.
//   * The null vector is the column of V whose column of A V has the smallest norm among the first `cols` (the first on a tie).
// The 4x4 method of kb8_triangulate.h (kb8_rotate) states the same rotation for the triangulation kernels and stays there.
#pragma once
#include "kb8_triangulate.h"

namespace osh {

constexpr int kJacobiSweeps = 10;   // 8 sweeps agreed with LAPACK's FP64 SVD to 3e-13 on 8-point sets of general and planar scenes, 6 did not
constexpr int kJacobiRows = 16;     // rows of a row array: the lanes the device adds across

// The rotation of one column pair from the three sums (as kb8_rotate)
OSH_KB8_HD void jacobi_rotation(double alpha, double beta, double gamma, double& c, double& s) {
#pragma clang fp contract(off)
  const double zeta = (beta - alpha) / (2.0 * gamma);
  double t = (zeta < 0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  if (gamma == 0.0 || !(t == t)) t = 0.0;
  c = 1.0 / sqrt(1.0 + t * t); s = c * t;
}
OSH_KB8_HD void jacobi_rotate_pair(double& xp, double& xq, double c, double s) {
#pragma clang fp contract(off)
  const double p = xp, q = xq;
  xp = c * p - s * q; xq = s * p + c * q;
}
// The pairwise tree over the 16 rows: what four xor-butterfly steps across 16 lanes leave in every one of them
OSH_KB8_HD double tree16(const double x[kJacobiRows]) {
#pragma clang fp contract(off)
  double t[kJacobiRows];
  for (int i = 0; i < kJacobiRows; ++i) t[i] = x[i];
  for (int w = 1; w < kJacobiRows; w *= 2)
    for (int i = 0; i < kJacobiRows; i += 2 * w) t[i] = t[i] + t[i + w];
  return t[0];
}
// The null vector of a 16 x COLS row array (rotated in place), plain C++: the kernels run the same operations with a row per lane
template <int COLS, int SWEEPS>
inline void null_vector(double a[kJacobiRows][COLS], int cols, double h[COLS]) {
#pragma clang fp contract(off)
  double v[COLS][COLS], x[kJacobiRows], y[kJacobiRows], z[kJacobiRows];
  for (int i = 0; i < COLS; ++i) for (int j = 0; j < COLS; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SWEEPS; ++sweep)
    for (int p = 0; p < COLS - 1; ++p)
      for (int q = p + 1; q < COLS; ++q) {
        for (int i = 0; i < kJacobiRows; ++i) { x[i] = a[i][p] * a[i][p]; y[i] = a[i][q] * a[i][q]; z[i] = a[i][p] * a[i][q]; }
        double c, s;
        jacobi_rotation(tree16(x), tree16(y), tree16(z), c, s);
        for (int i = 0; i < kJacobiRows; ++i) jacobi_rotate_pair(a[i][p], a[i][q], c, s);
        for (int i = 0; i < COLS; ++i) jacobi_rotate_pair(v[i][p], v[i][q], c, s);
      }
  int best = 0;
  double best_n = 0;
  for (int j = 0; j < cols; ++j) {
    for (int i = 0; i < kJacobiRows; ++i) x[i] = a[i][j] * a[i][j];
    const double n = tree16(x);
    if (j == 0 || n < best_n) { best_n = n; best = j; }
  }
  for (int k = 0; k < COLS; ++k) h[k] = v[k][best];
}

// One pair of a 3x3 matrix: b = A V, sums in row order
template <int P, int Q>
OSH_KB8_HD void jacobi_rotate3(double (&b)[3][3], double (&v)[3][3]) {
#pragma clang fp contract(off)
  double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { alpha += b[i][P] * b[i][P]; beta += b[i][Q] * b[i][Q]; gamma += b[i][P] * b[i][Q]; }
  double c, s;
  jacobi_rotation(alpha, beta, gamma, c, s);
#pragma unroll
  for (int i = 0; i < 3; ++i) { jacobi_rotate_pair(b[i][P], b[i][Q], c, s); jacobi_rotate_pair(v[i][P], v[i][Q], c, s); }
}

#ifdef __HIPCC__
__device__ __forceinline__ double rows_sum(double x) {   // tree16 over lanes 0..15, the result in every lane
#pragma clang fp contract(off)
  x = x + __shfl_xor(x, 1);
  x = x + __shfl_xor(x, 2);
  x = x + __shfl_xor(x, 4);
  x = x + __shfl_xor(x, 8);
  return __shfl(x, 0);
}
// null_vector by one wavefront.  row: lane l < 16 holds row l of the array, lane 16 + k row k of the identity (V), the other lanes
// zeros.  The pairs of a sweep are unrolled so that the rows stay in registers.  Returns the lane's entry of the chosen column: entry
// k of the null vector is __shfl(that, 16 + k).
template <int COLS, int SWEEPS>
__device__ __forceinline__ double null_vector_wave(double (&row)[COLS], int cols) {
#pragma clang fp contract(off)
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < COLS - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < COLS; ++q) {
        const double alpha = rows_sum(row[p] * row[p]), beta = rows_sum(row[q] * row[q]), gamma = rows_sum(row[p] * row[q]);
        double c, s;
        jacobi_rotation(alpha, beta, gamma, c, s);
        jacobi_rotate_pair(row[p], row[q], c, s);
      }
  }
  int best = 0;
  double best_n = 0;
#pragma unroll
  for (int j = 0; j < COLS; ++j) {
    const double nj = rows_sum(row[j] * row[j]);
    if (j < cols && (j == 0 || nj < best_n)) { best_n = nj; best = j; }
  }
  double mine = 0;
#pragma unroll
  for (int j = 0; j < COLS; ++j) if (j == best) mine = row[j];
  return mine;
}
#endif

}  // namespace osh
