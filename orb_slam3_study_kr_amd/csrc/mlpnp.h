// mlpnp.h -- MLPnPsolver (src/MLPnPsolver.cpp), the PnP RANSAC of Tracking::Relocalization: computePose (:356-658), rodrigues2rot
// (:660-675), rot2rodrigues (:677-692), mlpnp_gn (:694-758) with its residuals and Jacobian, CheckInliers (:262-293), and the record
// and Refine bookkeeping of iterate (:169-222) behind its minimal-set draw.  Device code of mlpnp_device.hip; plain C++ as well:
// ml_solve_host at the end is the whole pipeline on one thread (the host build the test library, the make target mlpnp-check and the
// drop-in's fall-back run).
//
// The solver is FP64 as in the reference, every statement a single IEEE operation with contraction off; CheckInliers is the
// reference's: xc, yc, zc formed in double from the pose and the float point, left to right, rounded to float once, then the camera's
// float project (Pinhole: fx * x / z + cx; KannalaBrandt8: kb8_project of kb8_triangulate.h), float error2 and error2 < max_error.
// covs(1) never has the size of the correspondences, so P is the identity and there is no covariance path.
//
// What is defined here and not by the reference (Eigen is not available, so parity with it is unpinned):
//   * The null space of a bearing vector f is columns 1 and 2 of the Householder reflection that maps f onto the first axis
//     (ml_nullspace), not Eigen's JacobiSVD.  A^T A, J^T J and J^T r depend only on N N^T = I - f f^T / |f|^2; the 1e-5 stop test of
//     mlpnp_gn is the only consumer of the basis itself.
//   * The rank of planarTest: column-pivoted Householder QR (the column of the largest remaining norm first), pivots counted while
//     |pivot| > 3 * eps * |largest pivot|, Eigen's default threshold for a 3x3 matrix (ml_rank3).
//   * The eigenvectors of planarTest (ascending eigenvalues), the null vector of the 12x12 or 9x9 normal matrix and the polar factor
//     U V^T of a 3x3 matrix come from the one-sided Jacobi method of jacobi_rows.h (jacobi_rotate3, null_vector) in FP64 with a fixed
//     number of sweeps.  The normal matrix is a row array there (rows 12..15 are zero); its null vector is taken among the first 12
//     or 9 columns.
//   * Every sum over the correspondences (planarTest, the normal matrix, J^T J, J^T r) is 64 partial sums, partial l adding the
//     correspondences l, l + 64, .. in that order, joined by the pairwise tree over the 64 (ml_tree64): the same for 6 and for 2048
//     correspondences, whatever the launch.  The normal matrix is kept as its 60 distinct sums Q[r][r'] * ([p;1][p;1]^T)[a][a'].
//   * The 6x6 solve is an unpivoted LDL^T (ml_ldlt6); the inverse of [R | t] is [R^T | -R^T t]; the cube root is pow(x, 1.0 / 3.0).
//   * The 2x6 Jacobian of N^T normalize(R(w) X + t) is analytic: with y = R X + t, u = y / |y|,
//     du/dt = (I - u u^T) / |y| and du/dw = du/dt * (-[R X]x Jl(w)), Jl(w) = I + (1 - cos a) / a^2 [w]x + (a - sin a) / a^3 [w]x^2
//     the left Jacobian of SO(3), a = |w|; for a <= eps, where rodrigues2rot returns the identity, Jl = I.  (The reference's generated
//     expressions divide by a there.)
//   * mlpnp_gn's tests on dx: a NaN in dx makes both `max|dx| > 5` and `min|dx| > 1` false, and `max|J dx| < 1e-5` is "every |J dx|
//     entry < 1e-5", false for a NaN, so the loop goes on to its bound of 5.
// No loop here depends on a convergence test: every bound is fixed, a NaN input ends in 0 inliers.
#pragma once
#include "jacobi_rows.h"
#include "ransac_stage.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace osh {

constexpr int kMlWave = 64;      // partial sums of a sum over the correspondences
constexpr int kMlSweeps = 12;    // Jacobi sweeps over the 66 column pairs of the 12x12 normal matrix
constexpr int kMlRows = kJacobiRows;   // rows of the normal matrix as a row array: 12 and four of zeros
constexpr int kMlGnIterations = 5;
constexpr double kMlEps = 2.220446049250313e-16;

struct MlProblem {
  int camera_type;
  float cam[8];
  int n, n_iter, min_inliers, best_in, ok_in;
  int words;            // mask words of one pose: 2 * ceil(n / 64)
  int base_p, base_h;   // offsets of the problem's correspondences and iterations in the arrays of the batch
  int base_w;           // offset of its iterations' mask words
};
struct MlHead {
  int first_hit, hit_record, hit_count, best_iteration, best_count, best_refine_ok, n_records, pad;
  double hit_pose[12], best_pose[12];
};

// ---------------------------------------------------------------------------------------------------- index maps
OSH_KB8_HD constexpr int ml_sym(int n, int a, int b) { return a <= b ? a * n - a * (a - 1) / 2 + (b - a) : b * n - b * (b - 1) / 2 + (a - b); }
// column k of the 12-column design matrix: rotation row r and coordinate a of [p; 1] (a = 3: the translation columns)
OSH_KB8_HD constexpr int ml_col_r(int k) { return k < 9 ? k / 3 : k - 9; }
OSH_KB8_HD constexpr int ml_col_a(int k) { return k < 9 ? k % 3 : 3; }
// column k of the planar 9-column design matrix as a column of the 12-column one: r12 r13 r22 r23 r32 r33 t1 t2 t3
OSH_KB8_HD constexpr int ml_planar_col(int k) { return k < 6 ? (k / 2) * 3 + 1 + (k & 1) : k + 3; }
// entry (row, col) of A^T A (planar: of the 9x9 one, zero beyond it) from the 60 sums T[q * 10 + p]
OSH_KB8_HD double ml_system_entry(const double* T, bool planar, int row, int col) {
  const int cols = planar ? 9 : 12;
  if (row >= cols || col >= cols) return 0.0;
  const int k = planar ? ml_planar_col(row) : row, l = planar ? ml_planar_col(col) : col;
  return T[ml_sym(3, ml_col_r(k), ml_col_r(l)) * 10 + ml_sym(4, ml_col_a(k), ml_col_a(l))];
}

// ---------------------------------------------------------------------------------------------------- small FP64 algebra
inline double ml_tree64(const double x[kMlWave]) {   // what six xor-butterfly steps across 64 lanes leave in every one of them
#pragma clang fp contract(off)
  double t[kMlWave];
  for (int i = 0; i < kMlWave; ++i) t[i] = x[i];
  for (int w = 1; w < kMlWave; w *= 2)
    for (int i = 0; i < kMlWave; i += 2 * w) t[i] = t[i] + t[i + w];
  return t[0];
}
OSH_KB8_HD void ml_mulv3(const double* A, const double* v, double* r) {   // r must not alias v
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
OSH_KB8_HD void ml_mulTv3(const double* A, const double* v, double* r) {   // A^T v
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
OSH_KB8_HD void ml_mul3(const double* A, const double* B, double* C) {   // C must not alias A or B
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
OSH_KB8_HD double ml_norm3(const double* v) {
#pragma clang fp contract(off)
  return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}
OSH_KB8_HD double ml_det3(const double* m) {
#pragma clang fp contract(off)
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// Columns 1 and 2 of H = I - 2 v v^T / (v^T v), v = f + sign(f0) |f| e0: an orthonormal basis of the plane orthogonal to f
OSH_KB8_HD void ml_nullspace(const double* f, double N[3][2]) {
#pragma clang fp contract(off)
  const double a = ml_norm3(f);
  const double v0 = f[0] + (f[0] < 0 ? -a : a), v1 = f[1], v2 = f[2];
  const double beta = 2.0 / (v0 * v0 + v1 * v1 + v2 * v2);
  N[0][0] = -(beta * v0 * v1); N[0][1] = -(beta * v0 * v2);
  N[1][0] = 1.0 - beta * v1 * v1; N[1][1] = -(beta * v1 * v2);
  N[2][0] = -(beta * v2 * v1); N[2][1] = 1.0 - beta * v2 * v2;
}
// N N^T as its 6 distinct entries (ml_sym(3, r, r'))
OSH_KB8_HD void ml_projector(const double N[3][2], double Q[6]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = r; s < 3; ++s) Q[ml_sym(3, r, s)] = N[r][0] * N[s][0] + N[r][1] * N[s][1];
}

// The rank of the symmetric 3x3 matrix S (6 distinct entries, ml_sym(3, r, r')) as FullPivHouseholderQR::rank() counts it
OSH_KB8_HD int ml_rank3(const double S[6]) {
#pragma clang fp contract(off)
  double c0[3], c1[3], c2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { c0[i] = S[ml_sym(3, i, 0)]; c1[i] = S[ml_sym(3, i, 1)]; c2[i] = S[ml_sym(3, i, 2)]; }
  double d[3];
  // step 0: the column of the largest norm to the front
  {
    const double n0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2], n1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2],
                 n2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
    const int j = (n1 > n0 && n1 >= n2) ? 1 : (n2 > n0 && n2 > n1) ? 2 : 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a = c0[i], b = j == 1 ? c1[i] : c2[i];
      if (j == 1) { c0[i] = b; c1[i] = a; }
      if (j == 2) { c0[i] = b; c2[i] = a; }
    }
    const double norm = sqrt(j == 1 ? n1 : j == 2 ? n2 : n0);
    d[0] = norm;
    const double alpha = c0[0] >= 0 ? -norm : norm;
    const double v[3] = {c0[0] - alpha, c0[1], c0[2]};
    const double vtv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (vtv > 0) {
      const double s1 = 2.0 * (v[0] * c1[0] + v[1] * c1[1] + v[2] * c1[2]) / vtv, s2 = 2.0 * (v[0] * c2[0] + v[1] * c2[1] + v[2] * c2[2]) / vtv;
#pragma unroll
      for (int i = 0; i < 3; ++i) { c1[i] = c1[i] - s1 * v[i]; c2[i] = c2[i] - s2 * v[i]; }
    }
  }
  // step 1 on rows 1..2 of the two remaining columns
  {
    const double n1 = c1[1] * c1[1] + c1[2] * c1[2], n2 = c2[1] * c2[1] + c2[2] * c2[2];
    if (n2 > n1) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double a = c1[i]; c1[i] = c2[i]; c2[i] = a; }
    }
    const double norm = sqrt(n2 > n1 ? n2 : n1);
    d[1] = norm;
    const double alpha = c1[1] >= 0 ? -norm : norm;
    const double v[2] = {c1[1] - alpha, c1[2]};
    const double vtv = v[0] * v[0] + v[1] * v[1];
    if (vtv > 0) {
      const double s2 = 2.0 * (v[0] * c2[1] + v[1] * c2[2]) / vtv;
      c2[1] = c2[1] - s2 * v[0]; c2[2] = c2[2] - s2 * v[1];
    }
  }
  d[2] = fabs(c2[2]);
  double maxp = d[0];
  if (d[1] > maxp) maxp = d[1];
  if (d[2] > maxp) maxp = d[2];
  const double threshold = 3.0 * kMlEps * maxp;
  int rank = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) if (d[k] > threshold) ++rank;
  return rank;
}

// One-sided Jacobi on a 3x3 matrix: b = A V with orthogonal columns
OSH_KB8_HD void ml_jacobi3(const double* A, double (&b)[3][3], double (&v)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { b[i][j] = A[3 * i + j]; v[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) { jacobi_rotate3<0, 1>(b, v); jacobi_rotate3<0, 2>(b, v); jacobi_rotate3<1, 2>(b, v); }
}
// SelfAdjointEigenSolver(planarTest).eigenvectors()^T: row j of E is the eigenvector of the j-th smallest eigenvalue (stable order)
OSH_KB8_HD void ml_eig3_rows(const double S[6], double* E) {
#pragma clang fp contract(off)
  double A[9], b[3][3], v[3][3], n[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[3 * i + j] = S[ml_sym(3, i, j)];
  ml_jacobi3(A, b, v);
#pragma unroll
  for (int j = 0; j < 3; ++j) n[j] = b[0][j] * b[0][j] + b[1][j] * b[1][j] + b[2][j] * b[2][j];
  int o0 = 0, o1 = 1, o2 = 2;
  if (n[1] < n[0]) { o0 = 1; o1 = 0; }
  {
    const double a0 = o0 == 0 ? n[0] : n[1], a1 = o1 == 0 ? n[0] : n[1];
    if (n[2] < a1) { o2 = o1; o1 = 2; if (n[2] < a0) { o1 = o0; o0 = 2; } }
  }
  const int order[3] = {o0, o1, o2};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k = order[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) E[3 * j + i] = k == 0 ? v[i][0] : k == 1 ? v[i][1] : v[i][2];
  }
}
// U V^T of A = U S V^T: sum over the columns j of (b_j / |b_j|) v_j^T
OSH_KB8_HD void ml_polar3(const double* A, double* R) {
#pragma clang fp contract(off)
  double b[3][3], v[3][3], n[3];
  ml_jacobi3(A, b, v);
#pragma unroll
  for (int j = 0; j < 3; ++j) n[j] = sqrt(b[0][j] * b[0][j] + b[1][j] * b[1][j] + b[2][j] * b[2][j]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) R[3 * i + k] = (b[i][0] / n[0]) * v[k][0] + (b[i][1] / n[1]) * v[k][1] + (b[i][2] / n[2]) * v[k][2];
}

// :660-675 and the left Jacobian of SO(3) beside it
OSH_KB8_HD void ml_rodrigues2rot(const double* w, double* R, double* Jl) {
#pragma clang fp contract(off)
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double W2[9];
  ml_mul3(W, W, W2);
  const double a = ml_norm3(w);
#pragma unroll
  for (int k = 0; k < 9; ++k) { R[k] = (k % 4 == 0) ? 1.0 : 0.0; Jl[k] = R[k]; }
  if (a > kMlEps) {
    const double s = sin(a), c = cos(a);
    const double k1 = s / a, k2 = (1 - c) / (a * a), k3 = (a - s) / (a * a * a);
#pragma unroll
    for (int k = 0; k < 9; ++k) { R[k] = R[k] + k1 * W[k] + k2 * W2[k]; Jl[k] = Jl[k] + k2 * W[k] + k3 * W2[k]; }
  }
}
// :677-692.  acos of a value outside [-1, 1] is NaN, `wnorm > eps` is then false and omega stays 0
OSH_KB8_HD void ml_rot2rodrigues(const double* R, double* omega) {
#pragma clang fp contract(off)
  omega[0] = omega[1] = omega[2] = 0.0;
  const double trace = R[0] + R[4] + R[8] - 1.0;
  const double wnorm = acos(trace / 2.0);
  if (wnorm > kMlEps) {
    const double sc = wnorm / (2.0 * sin(wnorm));
    omega[0] = (R[7] - R[5]) * sc; omega[1] = (R[2] - R[6]) * sc; omega[2] = (R[3] - R[1]) * sc;
  }
}

// ---------------------------------------------------------------------------------------------------- computePose: the sums
// planarTest = points3 * points3^T, one correspondence's share
OSH_KB8_HD void ml_add_planar(const double* p, double S[6]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = r; s < 3; ++s) S[ml_sym(3, r, s)] = S[ml_sym(3, r, s)] + p[r] * p[s];
}
// A^T A, one correspondence's share: T[q * 10 + a] += Q[q] * ([pt; 1][pt; 1]^T)[a]; pt = eigenRot * p in the planar case
OSH_KB8_HD void ml_add_system(const double* f, const double* p, bool planar, const double* E, double T[60]) {
#pragma clang fp contract(off)
  double N[3][2], Q[6], ph[4];
  ml_nullspace(f, N);
  ml_projector(N, Q);
  if (planar) ml_mulv3(E, p, ph); else { ph[0] = p[0]; ph[1] = p[1]; ph[2] = p[2]; }
  ph[3] = 1.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b) {
      const double pp = ph[a] * ph[b];
#pragma unroll
      for (int q = 0; q < 6; ++q) T[q * 10 + ml_sym(4, a, b)] = T[q * 10 + ml_sym(4, a, b)] + Q[q] * pp;
    }
}

// The null vector of the 16x12 array of rows (rows 12..15 and, planar, rows and columns 9..11 zero) among the first `cols` columns
inline void ml_null12(double a[kMlRows][12], int cols, double h[12]) { null_vector<12, kMlSweeps>(a, cols, h); }

// ---------------------------------------------------------------------------------------------------- computePose: :526-637
// h: the null vector (planar: 9 entries).  E: eigenRot (rows: eigenvectors), read when planar.  f6, p6: the first six correspondences.
// Out: Rout, tout as they enter the Gauss-Newton.
OSH_KB8_HD void ml_initial_pose(bool planar, const double* h, const double* E, const double* f6, const double* p6, double* Rout, double* tout) {
#pragma clang fp contract(off)
  if (planar) {
    // tmp << 0 h0 h1, 0 h2 h3, 0 h4 h5; tmp.col(0) = tmp.col(1).cross(tmp.col(2)); transposeInPlace
    const double c1[3] = {h[0], h[2], h[4]}, c2[3] = {h[1], h[3], h[5]};
    const double c0[3] = {c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0]};
    const double tmp[9] = {c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]};
    const double col1[3] = {tmp[1], tmp[4], tmp[7]}, col2[3] = {tmp[2], tmp[5], tmp[8]};
    const double scale = 1.0 / sqrt(fabs(ml_norm3(col1) * ml_norm3(col2)));
    double P[9], M[9];
    ml_polar3(tmp, P);
    if (ml_det3(P) < 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) P[k] = P[k] * -1.0;
    }
    // Rout1 = eigenRot^T * Rout1; transposeInPlace; *= -1
    double Et[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Et[3 * i + j] = E[3 * j + i];
    ml_mul3(Et, P, M);
    double R1[9], R2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R1[3 * i + j] = M[3 * j + i] * -1.0;
    if (ml_det3(R1) < 0.0) { R1[2] = R1[2] * -1.0; R1[5] = R1[5] * -1.0; R1[8] = R1[8] * -1.0; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { R2[3 * i] = -R1[3 * i]; R2[3 * i + 1] = -R1[3 * i + 1]; R2[3 * i + 2] = R1[3 * i + 2]; }
    const double t[3] = {scale * h[6], scale * h[7], scale * h[8]};
    int best = 0;
    double best_v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double* R = i < 2 ? R1 : R2;
      const double sg = (i & 1) ? -1.0 : 1.0;
      double norms = 0.0;
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        double y[3];
        ml_mulv3(R, p6 + 3 * p, y);
        y[0] = y[0] + sg * t[0]; y[1] = y[1] + sg * t[1]; y[2] = y[2] + sg * t[2];
        const double ny = ml_norm3(y);
        norms += 1.0 - ((y[0] / ny) * f6[3 * p] + (y[1] / ny) * f6[3 * p + 1] + (y[2] / ny) * f6[3 * p + 2]);
      }
      if (i == 0 || norms < best_v) { best_v = norms; best = i; }   // std::min_element: the first smallest
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Rout[k] = best < 2 ? R1[k] : R2[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tout[k] = (best & 1) ? -t[k] : t[k];
    return;
  }
  // tmp << h0 h3 h6, h1 h4 h7, h2 h5 h8
  const double tmp[9] = {h[0], h[3], h[6], h[1], h[4], h[7], h[2], h[5], h[8]};
  const double scale = 1.0 / pow(fabs(ml_norm3(h) * ml_norm3(h + 3) * ml_norm3(h + 6)), 1.0 / 3.0);
  double P[9];
  ml_polar3(tmp, P);
  if (ml_det3(P) < 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) P[k] = P[k] * -1.0;
  }
  const double ts[3] = {scale * h[9], scale * h[10], scale * h[11]};
  double t[3];
  ml_mulv3(P, ts, t);
  // Ts[s] = [P | +-t]^-1 = [P^T | -P^T (+-t)]
  double ti[3], err[2];
  ml_mulTv3(P, t, ti);
#pragma unroll
  for (int k = 0; k < 9; ++k) Rout[k] = P[3 * (k % 3) + k / 3];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double sg = s == 0 ? -1.0 : 1.0;   // the translation of Ts[s] is sg * ti
    err[s] = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      double y[3];
      ml_mulv3(Rout, p6 + 3 * p, y);
      y[0] = y[0] + sg * ti[0]; y[1] = y[1] + sg * ti[1]; y[2] = y[2] + sg * ti[2];
      const double ny = ml_norm3(y);
      err[s] += 1.0 - ((y[0] / ny) * f6[3 * p] + (y[1] / ny) * f6[3 * p + 1] + (y[2] / ny) * f6[3 * p + 2]);
    }
  }
  const double sg = err[0] < err[1] ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) tout[k] = sg * ti[k];
}

// ---------------------------------------------------------------------------------------------------- mlpnp_gn (:694-758)
struct MlGn { double R[9], Jl[9], t[3]; };
OSH_KB8_HD void ml_gn_setup(const double* x, MlGn& g) {
  ml_rodrigues2rot(x, g.R, g.Jl);
  g.t[0] = x[3]; g.t[1] = x[4]; g.t[2] = x[5];
}
// r = N^T u and its 2x6 Jacobian for one correspondence, u = normalize(R p + t)
OSH_KB8_HD void ml_gn_point(const MlGn& g, const double* f, const double* p, double J[2][6], double r[2]) {
#pragma clang fp contract(off)
  double N[3][2], Rp[3], y[3], u[3];
  ml_nullspace(f, N);
  ml_mulv3(g.R, p, Rp);
  y[0] = Rp[0] + g.t[0]; y[1] = Rp[1] + g.t[1]; y[2] = Rp[2] + g.t[2];
  const double ny = ml_norm3(y);
  u[0] = y[0] / ny; u[1] = y[1] / ny; u[2] = y[2] / ny;
  // dy/dw = -[Rp]x Jl
  const double C[9] = {0.0, -Rp[2], Rp[1], Rp[2], 0.0, -Rp[0], -Rp[1], Rp[0], 0.0};
  double A[9];
  ml_mul3(C, g.Jl, A);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double nu = N[0][c] * u[0] + N[1][c] * u[1] + N[2][c] * u[2];
    r[c] = nu;
    double m[3];   // (I - u u^T) N_c / |y|
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = (N[k][c] - u[k] * nu) / ny;
#pragma unroll
    for (int k = 0; k < 3; ++k) { J[c][k] = -(m[0] * A[k] + m[1] * A[3 + k] + m[2] * A[6 + k]); J[c][3 + k] = m[k]; }
  }
}
// J^T J (21 distinct entries, ml_sym(6, a, b)) and J^T r, one correspondence's share: H[0..20], H[21..26]
OSH_KB8_HD void ml_add_normal(const MlGn& g, const double* f, const double* p, double H[27]) {
#pragma clang fp contract(off)
  double J[2][6], r[2];
  ml_gn_point(g, f, p, J, r);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) H[ml_sym(6, a, b)] = H[ml_sym(6, a, b)] + (J[0][a] * J[0][b] + J[1][a] * J[1][b]);
    H[21 + a] = H[21 + a] + (J[0][a] * r[0] + J[1][a] * r[1]);
  }
}
// Both entries of J dx below 1e-5 for this correspondence
OSH_KB8_HD bool ml_update_small(const MlGn& g, const double* f, const double* p, const double* dx) {
#pragma clang fp contract(off)
  double J[2][6], r[2];
  ml_gn_point(g, f, p, J, r);
  bool small = true;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    double dl = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) dl += J[c][a] * dx[a];
    small = small && (fabs(dl) < 1e-5);
  }
  return small;
}
// dx of (J^T J) dx = J^T r by an unpivoted LDL^T
OSH_KB8_HD void ml_ldlt6(const double H[27], double dx[6]) {
#pragma clang fp contract(off)
  double L[6][6], D[6], y[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = H[ml_sym(6, j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k] * D[k];
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = H[ml_sym(6, i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k] * D[k];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = H[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * dx[k];
    dx[i] = s;
  }
}
// :744: true = break without the update
OSH_KB8_HD bool ml_gn_spurious(const double* dx) {
  bool nan = false;
  double mx = fabs(dx[0]), mn = fabs(dx[0]);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double v = fabs(dx[a]);
    nan = nan || !(v == v);
    if (v > mx) mx = v;
    if (v < mn) mn = v;
  }
  return !nan && (mx > 5.0 || mn > 1.0);
}

// ---------------------------------------------------------------------------------------------------- CheckInliers (:262-293)
OSH_KB8_HD bool ml_inlier(int camera_type, const float* cam, const double* T, const double* p3d, const float* p2d, float max_error) {
#pragma clang fp contract(off)
  const float X = (float)p3d[0], Y = (float)p3d[1], Z = (float)p3d[2];
  const float v[3] = {(float)(T[0] * (double)X + T[1] * (double)Y + T[2] * (double)Z + T[9]),
                      (float)(T[3] * (double)X + T[4] * (double)Y + T[5] * (double)Z + T[10]),
                      (float)(T[6] * (double)X + T[7] * (double)Y + T[8] * (double)Z + T[11])};
  const Pixel uv = ransac_project(camera_type, cam, v);
  const float distX = p2d[0] - uv.u, distY = p2d[1] - uv.v;
  const float error2 = distX * distX + distY * distY;
  return error2 < max_error;
}

// ---------------------------------------------------------------------------------------------------- iterate (:169-222)
// The records: iteration k is one when count[k] >= min_inliers and count[k] > the running best, which starts at best_in
OSH_KB8_HD int ml_scan_records(const int* count, int n_iter, int min_inliers, int best_in, int* record) {
  int best = best_in, n_rec = 0;
  for (int k = 0; k < n_iter; ++k)
    if (count[k] >= min_inliers && count[k] > best) { best = count[k]; record[n_rec++] = k; }
  return n_rec;
}
// The decision: first_hit is the first k with count[k] >= min_inliers whose running best has a successful Refine (record_count >
// min_inliers; ok_in while no record has occurred), and the running best there, or after the last iteration without a hit
OSH_KB8_HD void ml_decide(const int* count, int n_iter, int min_inliers, int best_in, int ok_in, const int* record, const int* record_count,
                          MlHead& H) {
  int best = best_in, ok = ok_in ? 1 : 0, rec = -1, n_rec = 0, hit = -1;
  for (int k = 0; k < n_iter && hit < 0; ++k)
    if (count[k] >= min_inliers) {
      if (count[k] > best) { best = count[k]; rec = n_rec++; ok = record_count[rec] > min_inliers ? 1 : 0; }
      if (ok) hit = k;
    }
  H.first_hit = hit;
  H.hit_record = hit >= 0 ? rec : -1;
  H.hit_count = hit >= 0 && rec >= 0 ? record_count[rec] : 0;
  H.best_iteration = rec >= 0 ? record[rec] : -1;
  H.best_count = best;
  H.best_refine_ok = ok;
}

// SetRansacParameters (:225-260): mRansacMinInliers and mRansacMaxIts for N correspondences.  epsilon is a float as in the reference;
// pow(epsilon, 3) is the double power of the float
inline void ml_ransac_parameters(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon, int* min_inliers,
                                 int* max_iterations) {
  int nMinInliers = (int)((float)N * epsilon);
  if (nMinInliers < minInliers) nMinInliers = minInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  if (N > 0 && epsilon < (float)nMinInliers / (float)N) epsilon = (float)nMinInliers / (float)N;
  int nIterations = 1;
  if (nMinInliers != N) {
    const double v = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3)));
    nIterations = v == v && v > -2147483648.0 && v < 2147483647.0 ? (int)v : INT32_MIN;   // what the conversion gives on x86-64
  }
  *min_inliers = nMinInliers;
  *max_iterations = std::max(1, std::min(nIterations, maxIterations));
}

// ---------------------------------------------------------------------------------------------------- the host build
// computePose over the correspondences idx[0..n) of (bearing, p3d): pose = R (row-major), t.  info (may be null): planar, Gauss-Newton
// updates applied, how the Gauss-Newton ended (0: its bound, 1: the break of :744, 2: the stop of :748).
inline void ml_gauss_newton_host(int n, const int* idx, const double* bearing, const double* p3d, double x[6], int max_iterations, int* info) {
#pragma clang fp contract(off)
  int updates = 0, reason = 0;
  for (int it = 0; it < max_iterations; ++it) {
    MlGn g;
    ml_gn_setup(x, g);
    double part[27][kMlWave], H[27], dx[6];
    for (int l = 0; l < kMlWave; ++l) {
      double h[27];
      for (int k = 0; k < 27; ++k) h[k] = 0.0;
      for (int i = l; i < n; i += kMlWave) ml_add_normal(g, bearing + 3 * (size_t)idx[i], p3d + 3 * (size_t)idx[i], h);
      for (int k = 0; k < 27; ++k) part[k][l] = h[k];
    }
    for (int k = 0; k < 27; ++k) H[k] = ml_tree64(part[k]);
    ml_ldlt6(H, dx);
    if (ml_gn_spurious(dx)) { reason = 1; break; }
    bool small = true;
    for (int i = 0; i < n; ++i) small = ml_update_small(g, bearing + 3 * (size_t)idx[i], p3d + 3 * (size_t)idx[i], dx) && small;
    for (int k = 0; k < 6; ++k) x[k] = x[k] - dx[k];
    ++updates;
    if (small) { reason = 2; break; }
  }
  if (info) { info[1] = updates; info[2] = reason; }
}
inline void ml_compute_pose_host(int n, const int* idx, const double* bearing, const double* p3d, double pose[12], int* info) {
#pragma clang fp contract(off)
  double S[6], E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  {
    double part[6][kMlWave];
    for (int l = 0; l < kMlWave; ++l) {
      double s[6] = {0, 0, 0, 0, 0, 0};
      for (int i = l; i < n; i += kMlWave) ml_add_planar(p3d + 3 * (size_t)idx[i], s);
      for (int k = 0; k < 6; ++k) part[k][l] = s[k];
    }
    for (int k = 0; k < 6; ++k) S[k] = ml_tree64(part[k]);
  }
  const bool planar = ml_rank3(S) == 2;
  if (planar) ml_eig3_rows(S, E);
  double T[60];
  {
    static thread_local double part[60][kMlWave];
    for (int l = 0; l < kMlWave; ++l) {
      double t[60];
      for (int k = 0; k < 60; ++k) t[k] = 0.0;
      for (int i = l; i < n; i += kMlWave) ml_add_system(bearing + 3 * (size_t)idx[i], p3d + 3 * (size_t)idx[i], planar, E, t);
      for (int k = 0; k < 60; ++k) part[k][l] = t[k];
    }
    for (int k = 0; k < 60; ++k) T[k] = ml_tree64(part[k]);
  }
  double a[kMlRows][12], h[12];
  for (int i = 0; i < kMlRows; ++i) for (int j = 0; j < 12; ++j) a[i][j] = i < 12 ? ml_system_entry(T, planar, i, j) : 0.0;
  ml_null12(a, planar ? 9 : 12, h);
  double f6[18], p6[18], R[9], x[6];
  for (int p = 0; p < 6; ++p) for (int k = 0; k < 3; ++k) { f6[3 * p + k] = bearing[3 * (size_t)idx[p] + k]; p6[3 * p + k] = p3d[3 * (size_t)idx[p] + k]; }
  ml_initial_pose(planar, h, E, f6, p6, R, x + 3);
  ml_rot2rodrigues(R, x);
  if (info) info[0] = planar ? 1 : 0;
  ml_gauss_newton_host(n, idx, bearing, p3d, x, kMlGnIterations, info);
  double Jl[9];
  ml_rodrigues2rot(x, pose, Jl);
  pose[9] = x[3]; pose[10] = x[4]; pose[11] = x[5];
}
// CheckInliers of one pose over the n correspondences: the count, the mask as bit words (bit i % 32 of word i / 32)
inline int ml_check_inliers_host(const osh_mlpnp_problem& P, const double* pose, uint32_t* mask) {
  const int words = ransac_mask_words(P.n);
  int count = 0;
  for (int w = 0; w < words; ++w) mask[w] = 0;
  for (int i = 0; i < P.n; ++i)
    if (ml_inlier(P.camera_type, P.camera, pose, P.p3d + 3 * (size_t)i, P.p2d + 2 * (size_t)i, P.max_error[i])) { mask[i >> 5] |= 1u << (i & 31); ++count; }
  return count;
}

template <class T>
inline void ml_zero(T* dst, size_t n) { if (dst && n) std::memset(dst, 0, n * sizeof(T)); }
inline void ml_write_head(const osh_mlpnp_result& r, const MlHead& H) {
  if (r.first_hit) *r.first_hit = H.first_hit;
  if (r.hit_record) *r.hit_record = H.hit_record;
  if (r.hit_count) *r.hit_count = H.hit_count;
  if (r.best_iteration) *r.best_iteration = H.best_iteration;
  if (r.best_count) *r.best_count = H.best_count;
  if (r.best_refine_ok) *r.best_refine_ok = H.best_refine_ok;
  if (r.n_records) *r.n_records = H.n_records;
  copy_if(r.hit_pose, H.hit_pose, 12);
  copy_if(r.best_pose, H.best_pose, 12);
}

// osh_orb_mlpnp_solve for one valid problem, on one thread
inline void ml_solve_host(const osh_mlpnp_problem& P, const osh_mlpnp_result& r) {
  const int n = P.n, n_it = P.n_iterations, words = ransac_mask_words(n);
  const size_t ni = (size_t)n_it;
  std::vector<double> pose(ni * 12 + 12), rec_pose(ni * 12 + 12);
  std::vector<int> count(ni + 1), record(ni + 1), rec_count(ni + 1), idx((size_t)n + 6);
  std::vector<uint32_t> mask(ni * words + 2), rec_mask(ni * words + 2);
  for (int k = 0; k < n_it; ++k) {
    ml_compute_pose_host(6, P.sets + 6 * (size_t)k, P.bearing, P.p3d, &pose[12 * (size_t)k], nullptr);
    count[k] = ml_check_inliers_host(P, &pose[12 * (size_t)k], &mask[(size_t)k * words]);
  }
  MlHead H;
  std::memset(&H, 0, sizeof(H));
  H.n_records = ml_scan_records(count.data(), n_it, P.min_inliers, P.best_inliers_in, record.data());
  for (int q = 0; q < H.n_records; ++q) {
    const uint32_t* m = &mask[(size_t)record[q] * words];
    int c = 0;
    for (int i = 0; i < n; ++i) if (m[i >> 5] >> (i & 31) & 1u) idx[c++] = i;
    ml_compute_pose_host(c, idx.data(), P.bearing, P.p3d, &rec_pose[12 * (size_t)q], nullptr);
    rec_count[q] = ml_check_inliers_host(P, &rec_pose[12 * (size_t)q], &rec_mask[(size_t)q * words]);
  }
  ml_decide(count.data(), n_it, P.min_inliers, P.best_inliers_in, P.best_refine_ok_in, record.data(), rec_count.data(), H);
  if (H.hit_record >= 0) std::memcpy(H.hit_pose, &rec_pose[12 * (size_t)H.hit_record], 96);
  if (H.best_iteration >= 0) std::memcpy(H.best_pose, &pose[12 * (size_t)H.best_iteration], 96);
  ml_write_head(r, H);
  if (H.hit_record >= 0) copy_if(r.hit_mask, &rec_mask[(size_t)H.hit_record * words], words); else ml_zero(r.hit_mask, words);
  if (H.best_iteration >= 0) copy_if(r.best_mask, &mask[(size_t)H.best_iteration * words], words); else ml_zero(r.best_mask, words);
  copy_if(r.debug_pose, pose.data(), ni * 12);
  copy_if(r.debug_count, count.data(), ni);
  for (size_t q = (size_t)H.n_records; q < ni; ++q) { record[q] = -1; rec_count[q] = 0; for (int k = 0; k < 12; ++k) rec_pose[12 * q + k] = 0.0; }
  copy_if(r.debug_record, record.data(), ni);
  copy_if(r.debug_record_count, rec_count.data(), ni);
  copy_if(r.debug_record_pose, rec_pose.data(), ni * 12);
}

}  // namespace osh
