// two_view.h -- TwoViewReconstruction (src/TwoViewReconstruction.cc:41-927), the monocular initialisation: Normalize (:737-784),
// ComputeH21 / ComputeF21 (:232-308), CheckHomography / CheckFundamental (:310-473), the RANSAC choice (:131-230), ReconstructH
// (:571-734), ReconstructF with DecomposeE (:475-569,903-927) and CheckRT (:786-901).  Device code of two_view_device.hip; plain C++
// as well: tv_reconstruct_host at the end is the whole pipeline on one thread (the host build the test library, the make target
// two-view-check and the drop-in's fall-back run).
//
// The parity rules of kb8_triangulate.h / newpoint_triangulate.h hold: single float32 operations in the reference's order with
// contraction off, Eigen's three-term reductions (3x3 products, dot, norm) as a0 + (a1 + a2), plain C++ expressions left to right,
// sqrt and acos as the FP64 function rounded once, double comparisons where the reference compares with a double literal,
// x = 1.0 / y as the double division rounded once.  What is defined here and not by the reference:
//   * Singular vectors come from the one-sided Jacobi method of jacobi_rows.h in FP64 on the float32 entries, kJacobiSweeps = 10
//     sweeps, no data-dependent loop.  The 16x9 (H) or 8x9 (F, rows 8..15 zero) system is a row array there: every sum over the rows
//     is the pairwise tree, and the null vector (null_vector<9, kJacobiSweeps>) is rounded to float32 once.
//   * The 3x3 SVD (rank 2 of F, DecomposeE, ReconstructH): the same method, 10 sweeps over (0,1) (0,2) (1,2), sums in row order;
//     singular values descending (stable); u0 = B0 / s0 and u1 = B1 / s1 of B = A * V (a zero vector for a zero singular value),
//     u2 = +-(u0 x u1) with the sign that makes u2 . B2 >= 0; everything rounded to float32 once.
//     Fn = B0 * v0^T + B1 * v1^T, which has no sign freedom, rounded to float32 once.
//   * tv_inverse3 (T2.inverse(), H21i.inverse(), K.inverse()) is the float32 cofactor inverse in the statement order written there;
//     tv_det3 is m00*(m11*m22 - m12*m21) - m01*(m10*m22 - m12*m20) + m02*(m10*m21 - m11*m20), left to right.
//   * The order statistic of CheckRT is taken in the total order of the float32 bit patterns (tv_cos_key), so that it is defined for
//     every input; on ordinary cosines it is std::sort's.
#pragma once
#include "jacobi_rows.h"
#include "../../include/orbslam3_hip.h"
#include <cstring>

namespace osh {

constexpr int kTvRows = kJacobiRows;   // rows of the system of a minimal set: 2 * 8 (H); F fills 8 and leaves the rest zero

struct TvProblem {
  float K[9], T1[9], T2[9];   // row-major
  float sigma;
  int n_iter, n_matches;
  int base_m, base_h;         // offsets of the problem's matches and of its iterations in the arrays of the batch
};
// What the select-and-decompose step leaves for CheckRT and the decision, and the head of a problem's result
struct TvHead {
  int status, best_h, best_f, branch, n_inliers, n_hyp, winner, pad;
  float T21[12], sh, sf, H21[9], F21[9];
  int n_good[8];
  float parallax[8];
  float R[8][9], t[8][3];
};

// ---------------------------------------------------------------------------------------------------- small float32 3x3 algebra
OSH_KB8_HD void tv_mul3(const float* A, const float* B, float* C) {   // C = A * B; C must not alias A or B
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = kb8_sum3(A[3 * i] * B[j], A[3 * i + 1] * B[3 + j], A[3 * i + 2] * B[6 + j]);
}
OSH_KB8_HD void tv_transpose3(const float* A, float* T) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * j + i];
}
OSH_KB8_HD void tv_mulv3(const float* A, const float* v, float* r) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = kb8_sum3(A[3 * i] * v[0], A[3 * i + 1] * v[1], A[3 * i + 2] * v[2]);
}
OSH_KB8_HD float tv_norm3(const float* v) {
#pragma clang fp contract(off)
  return kb8_sqrt(kb8_sum3(v[0] * v[0], v[1] * v[1], v[2] * v[2]));
}
OSH_KB8_HD float tv_det3(const float* m) {
#pragma clang fp contract(off)
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
OSH_KB8_HD void tv_inverse3(const float* m, float* inv) {
#pragma clang fp contract(off)
  const float c00 = m[4] * m[8] - m[5] * m[7];
  const float c01 = m[5] * m[6] - m[3] * m[8];
  const float c02 = m[3] * m[7] - m[4] * m[6];
  const float det = kb8_sum3(m[0] * c00, m[1] * c01, m[2] * c02);
  const float invdet = 1.f / det;
  inv[0] = c00 * invdet; inv[3] = c01 * invdet; inv[6] = c02 * invdet;
  inv[1] = (m[2] * m[7] - m[1] * m[8]) * invdet;
  inv[4] = (m[0] * m[8] - m[2] * m[6]) * invdet;
  inv[7] = (m[1] * m[6] - m[0] * m[7]) * invdet;
  inv[2] = (m[1] * m[5] - m[2] * m[4]) * invdet;
  inv[5] = (m[2] * m[3] - m[0] * m[5]) * invdet;
  inv[8] = (m[0] * m[4] - m[1] * m[3]) * invdet;
}

// ---------------------------------------------------------------------------------------------------- Normalize (:737-784)
// xy: all n keypoints of a frame, x y interleaved; pn: the same layout.  The sums are sequential float32 chains in index order.
OSH_KB8_HD void tv_normalize(const float* xy, int n, float* pn, float* T) {
#pragma clang fp contract(off)
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; i++) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
  meanX = meanX / (float)n; meanY = meanY / (float)n;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; i++) {
    pn[2 * i] = xy[2 * i] - meanX; pn[2 * i + 1] = xy[2 * i + 1] - meanY;
    meanDevX += fabsf(pn[2 * i]); meanDevY += fabsf(pn[2 * i + 1]);
  }
  meanDevX = meanDevX / (float)n; meanDevY = meanDevY / (float)n;
  const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
  for (int i = 0; i < n; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
  for (int k = 0; k < 9; ++k) T[k] = 0.f;
  T[0] = sX; T[4] = sY; T[2] = -meanX * sX; T[5] = -meanY * sY; T[8] = 1.f;
}

// ---------------------------------------------------------------------------------------------------- the systems (:232-308)
// Row r of A for a minimal set: model 0 = H (r = 2 * point + which), model 1 = F (r = point; rows 8..15 zero)
OSH_KB8_HD void tv_system_row(int model, int r, float u1, float v1, float u2, float v2, float a[9]) {
#pragma clang fp contract(off)
  if (model == 0) {
    if ((r & 1) == 0) { a[0] = 0.f; a[1] = 0.f; a[2] = 0.f; a[3] = -u1; a[4] = -v1; a[5] = -1.f; a[6] = v2 * u1; a[7] = v2 * v1; a[8] = v2; }
    else { a[0] = u1; a[1] = v1; a[2] = 1.f; a[3] = 0.f; a[4] = 0.f; a[5] = 0.f; a[6] = -u2 * u1; a[7] = -u2 * v1; a[8] = -u2; }
  } else if (r < 8) {
    a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1.f;
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = 0.f;
  }
}

// The null vector of a 16x9 system, rounded to float32 once
inline void tv_null9(const float A[kTvRows][9], float h[9]) {
  double a[kTvRows][9], hd[9];
  for (int i = 0; i < kTvRows; ++i) for (int j = 0; j < 9; ++j) a[i][j] = (double)A[i][j];
  null_vector<9, kJacobiSweeps>(a, 9, hd);
  for (int k = 0; k < 9; ++k) h[k] = (float)hd[k];
}

// ---------------------------------------------------------------------------------------------------- the 3x3 SVD
// M = U * diag(w) * V^T (row-major), w descending
OSH_KB8_HD void tv_svd3(const float* M, float* U, float* w, float* V) {
#pragma clang fp contract(off)
  double b[3][3], v[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { b[i][j] = (double)M[3 * i + j]; v[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) { jacobi_rotate3<0, 1>(b, v); jacobi_rotate3<0, 2>(b, v); jacobi_rotate3<1, 2>(b, v); }
  double n[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) n[j] = sqrt(b[0][j] * b[0][j] + b[1][j] * b[1][j] + b[2][j] * b[2][j]);
  // stable descending order of three
  int o0 = 0, o1 = 1, o2 = 2;
  if (n[o1] > n[o0]) { const int t = o0; o0 = o1; o1 = t; }
  if (n[o2] > n[o1]) { const int t = o1; o1 = o2; o2 = t; }
  if (n[o1] > n[o0]) { const int t = o0; o0 = o1; o1 = t; }
  const int order[3] = {o0, o1, o2};
  double B[3][3], Vs[3][3], s[3], u[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // order[j] as a select chain: the arrays stay in registers on the device
    const int k = order[j];
    s[j] = k == 0 ? n[0] : k == 1 ? n[1] : n[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      B[i][j] = k == 0 ? b[i][0] : k == 1 ? b[i][1] : b[i][2];
      Vs[i][j] = k == 0 ? v[i][0] : k == 1 ? v[i][1] : v[i][2];
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i][j] = s[j] == 0.0 ? 0.0 : B[i][j] / s[j];
  u[0][2] = u[1][0] * u[2][1] - u[2][0] * u[1][1];
  u[1][2] = u[2][0] * u[0][1] - u[0][0] * u[2][1];
  u[2][2] = u[0][0] * u[1][1] - u[1][0] * u[0][1];
  if (u[0][2] * B[0][2] + u[1][2] * B[1][2] + u[2][2] * B[2][2] < 0.0) { u[0][2] = -u[0][2]; u[1][2] = -u[1][2]; u[2][2] = -u[2][2]; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { U[3 * i + j] = (float)u[i][j]; V[3 * i + j] = (float)Vs[i][j]; }
  w[0] = (float)s[0]; w[1] = (float)s[1]; w[2] = (float)s[2];
}
// :302-307: the rank-2 matrix next to Fpre (h, row-major)
OSH_KB8_HD void tv_rank2(const float* Fpre, float* Fn) {
#pragma clang fp contract(off)
  double b[3][3], v[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { b[i][j] = (double)Fpre[3 * i + j]; v[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) { jacobi_rotate3<0, 1>(b, v); jacobi_rotate3<0, 2>(b, v); jacobi_rotate3<1, 2>(b, v); }
  double n[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) n[j] = b[0][j] * b[0][j] + b[1][j] * b[1][j] + b[2][j] * b[2][j];
  // drop the column of the smallest singular value (the last of the equal ones): Fn = sum over the other two of B_j * v_j^T
  int drop = 2;
  if (n[1] < n[drop]) drop = 1;
  if (n[0] < n[drop]) drop = 0;
  const int j0 = drop == 0 ? 1 : 0, j1 = drop == 2 ? 1 : 2;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double b0 = j0 == 0 ? b[i][0] : b[i][1], v0 = j0 == 0 ? v[j][0] : v[j][1];
      const double b1 = j1 == 1 ? b[i][1] : b[i][2], v1 = j1 == 1 ? v[j][1] : v[j][2];
      Fn[3 * i + j] = (float)(b0 * v0 + b1 * v1);
    }
}

// ---------------------------------------------------------------------------------------------------- model of a hypothesis
// h: the null vector.  model 0: Hn = h, H21i = T2inv * Hn * T1, H12i = H21i^-1.  model 1: Fn = rank2(h), F21i = T2^T * Fn * T1.
// T2x: T2inv (H) or T2^T (F).  out: normalised model, model, inverse (H; zeros for F).
OSH_KB8_HD void tv_model(int model, const float h[9], const float* T2x, const float* T1, float* Mn, float* M, float* Minv) {
#pragma clang fp contract(off)
  float tmp[9];
  if (model == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Mn[k] = h[k];
    tv_mul3(T2x, Mn, tmp); tv_mul3(tmp, T1, M);
    tv_inverse3(M, Minv);
  } else {
    tv_rank2(h, Mn);
    tv_mul3(T2x, Mn, tmp); tv_mul3(tmp, T1, M);
#pragma unroll
    for (int k = 0; k < 9; ++k) Minv[k] = 0.f;
  }
}
OSH_KB8_HD float tv_inv_sigma_square(float sigma) {
#pragma clang fp contract(off)
  return (float)(1.0 / (double)(sigma * sigma));
}

// ---------------------------------------------------------------------------------------------------- scoring (:310-473)
// The two terms match i adds to the score, in order (0 where the reference adds nothing: score + 0 is score); true: an inlier
OSH_KB8_HD bool tv_check_h(const float* H21, const float* H12, float invSigmaSquare, float u1, float v1, float u2, float v2, float& t1, float& t2) {
#pragma clang fp contract(off)
  const float th = 5.991f;
  bool bIn = true;
  const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
  const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
  const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) { bIn = false; t1 = 0.f; } else t1 = th - chiSquare1;
  const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
  const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
  const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) { bIn = false; t2 = 0.f; } else t2 = th - chiSquare2;
  return bIn;
}
OSH_KB8_HD bool tv_check_f(const float* F, float invSigmaSquare, float u1, float v1, float u2, float v2, float& t1, float& t2) {
#pragma clang fp contract(off)
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) { bIn = false; t1 = 0.f; } else t1 = thScore - chiSquare1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) { bIn = false; t2 = 0.f; } else t2 = thScore - chiSquare2;
  return bIn;
}
OSH_KB8_HD bool tv_check(int model, const float* M, const float* Minv, float invSigmaSquare, float u1, float v1, float u2, float v2, float& t1, float& t2) {
  return model == 0 ? tv_check_h(M, Minv, invSigmaSquare, u1, v1, u2, v2, t1, t2) : tv_check_f(M, invSigmaSquare, u1, v1, u2, v2, t1, t2);
}

// ---------------------------------------------------------------------------------------------------- motion hypotheses
// DecomposeE (:903-927) behind E21 = K^T * F21 * K (:484): (R1, t) (R2, t) (R1, -t) (R2, -t)
OSH_KB8_HD void tv_motion_f(const float* F21, const float* K, float R[8][9], float t[8][3]) {
#pragma clang fp contract(off)
  float Kt[9], tmp[9], E[9], U[9], V[9], w[3], Vt[9];
  tv_transpose3(K, Kt);
  tv_mul3(Kt, F21, tmp); tv_mul3(tmp, K, E);
  tv_svd3(E, U, w, V);
  tv_transpose3(V, Vt);
  float tt[3] = {U[2], U[5], U[8]};
  const float nt = tv_norm3(tt);
  tt[0] = tt[0] / nt; tt[1] = tt[1] / nt; tt[2] = tt[2] / nt;
  const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  float Wt[9], R1[9], R2[9];
  tv_transpose3(W, Wt);
  tv_mul3(U, W, tmp); tv_mul3(tmp, Vt, R1);
  if (tv_det3(R1) < 0) for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
  tv_mul3(U, Wt, tmp); tv_mul3(tmp, Vt, R2);
  if (tv_det3(R2) < 0) for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) { R[0][k] = R1[k]; R[1][k] = R2[k]; R[2][k] = R1[k]; R[3][k] = R2[k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) { t[0][k] = tt[k]; t[1][k] = tt[k]; t[2][k] = -tt[k]; t[3][k] = -tt[k]; }
}
// ReconstructH (:582-690).  False: d1 / d2 or d2 / d3 below 1.00001 (:597).
OSH_KB8_HD bool tv_motion_h(const float* H21, const float* K, float R[8][9], float t[8][3]) {
#pragma clang fp contract(off)
  float invK[9], tmp[9], A[9], U[9], V[9], w[3], Vt[9];
  tv_inverse3(K, invK);
  tv_mul3(invK, H21, tmp); tv_mul3(tmp, K, A);
  tv_svd3(A, U, w, V);
  tv_transpose3(V, Vt);
  const float s = tv_det3(U) * tv_det3(Vt);
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
  const float aux1 = kb8_sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = kb8_sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = kb8_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = kb8_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  float sU[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) sU[k] = s * U[k];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = i & 3;
    float Rp[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float tp[3];
    if (i < 4) {
      Rp[0] = ctheta; Rp[2] = -stheta[j]; Rp[4] = 1.f; Rp[6] = stheta[j]; Rp[8] = ctheta;
      tp[0] = x1[j] * (d1 - d3); tp[1] = 0.f * (d1 - d3); tp[2] = -x3[j] * (d1 - d3);
    } else {
      Rp[0] = cphi; Rp[2] = sphi[j]; Rp[4] = -1.f; Rp[6] = sphi[j]; Rp[8] = -cphi;
      tp[0] = x1[j] * (d1 + d3); tp[1] = 0.f * (d1 + d3); tp[2] = x3[j] * (d1 + d3);
    }
    tv_mul3(sU, Rp, tmp); tv_mul3(tmp, Vt, R[i]);
    float tt[3];
    tv_mulv3(U, tp, tt);
    const float nt = tv_norm3(tt);
    t[i][0] = tt[0] / nt; t[i][1] = tt[1] / nt; t[i][2] = tt[2] / nt;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------- CheckRT (:786-901)
struct TvCamera2 { float P2[12], O2[3]; };   // K * [R | t] and -R^T * t (:811-816)
OSH_KB8_HD void tv_camera2(const float* K, const float* R, const float* t, TvCamera2& c) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float b0 = j < 3 ? R[j] : t[0], b1 = j < 3 ? R[3 + j] : t[1], b2 = j < 3 ? R[6 + j] : t[2];
      c.P2[4 * i + j] = kb8_sum3(K[3 * i] * b0, K[3 * i + 1] * b1, K[3 * i + 2] * b2);
    }
    c.O2[i] = kb8_sum3(-R[i] * t[0], -R[3 + i] * t[1], -R[6 + i] * t[2]);
  }
}
OSH_KB8_HD bool tv_finite(float x) { return (x - x) == 0.f; }
// 0: the match is not counted; 1: counted (nGood, vCosParallax, vP3D); 2: counted and vbGood.  x3d, cosp: written when counted.
OSH_KB8_HD int tv_check_rt(const float* K, const float* R, const float* t, const TvCamera2& c, float th2, float u1, float v1, float u2, float v2,
                           float x3d[3], float& cosp) {
#pragma clang fp contract(off)
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  float A[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float p1_0 = j < 3 ? K[j] : 0.f, p1_1 = j < 3 ? K[3 + j] : 0.f, p1_2 = j < 3 ? K[6 + j] : 0.f;   // P1 = [K | 0]
    A[0][j] = u1 * p1_2 - p1_0;
    A[1][j] = v1 * p1_2 - p1_1;
    A[2][j] = u2 * c.P2[8 + j] - c.P2[j];
    A[3][j] = v2 * c.P2[8 + j] - c.P2[4 + j];
  }
  float p[3];
  kb8_null_vector(A, p);
  if (!tv_finite(p[0]) || !tv_finite(p[1]) || !tv_finite(p[2])) return 0;
  const float dist1 = tv_norm3(p);                                   // normal1 = p3dC1 - O1, O1 = 0
  const float n2[3] = {p[0] - c.O2[0], p[1] - c.O2[1], p[2] - c.O2[2]};
  const float dist2 = tv_norm3(n2);
  const float cosParallax = kb8_sum3(p[0] * n2[0], p[1] * n2[1], p[2] * n2[2]) / (dist1 * dist2);
  if (p[2] <= 0 && (double)cosParallax < 0.99998) return 0;
  float p2[3];
  tv_mulv3(R, p, p2);
  p2[0] = p2[0] + t[0]; p2[1] = p2[1] + t[1]; p2[2] = p2[2] + t[2];
  if (p2[2] <= 0 && (double)cosParallax < 0.99998) return 0;
  const float invZ1 = (float)(1.0 / (double)p[2]);
  const float im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
  const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
  if (squareError1 > th2) return 0;
  const float invZ2 = (float)(1.0 / (double)p2[2]);
  const float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
  const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
  if (squareError2 > th2) return 0;
  x3d[0] = p[0]; x3d[1] = p[1]; x3d[2] = p[2];
  cosp = cosParallax;
  return (double)cosParallax < 0.99998 ? 2 : 1;
}
OSH_KB8_HD float tv_th2(float sigma) {
#pragma clang fp contract(off)
  return (float)(4.0 * (double)(sigma * sigma));
}
// The total order of float32 bit patterns as unsigned keys (ascending key = ascending value) and back
OSH_KB8_HD unsigned tv_cos_key(float c) {
  unsigned u;
  memcpy(&u, &c, 4);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
OSH_KB8_HD float tv_key_cos(unsigned k) {
  const unsigned u = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
  float c;
  memcpy(&c, &u, 4);
  return c;
}
// :890-898 from the chosen cosine
OSH_KB8_HD float tv_parallax(float cosp) {
#pragma clang fp contract(off)
  const float a = (float)acos((double)cosp);
  return (float)((double)(a * 180.f) / 3.1415926535897932384626433832795);
}

// ---------------------------------------------------------------------------------------------------- the decisions
// ReconstructF :505-568 (branch 0) and ReconstructH :693-733 (branch 1) on the counts and parallaxes of the hypotheses.
// minParallax = 1.0, minTriangulated = 50 (:116,122,127).  winner: the hypothesis whose T21 / points are reported (-1: none).
OSH_KB8_HD int tv_decide(int branch, int N, const int* nGood, const float* parallax, int* winner) {
  const float minParallax = 1.0f;
  const int minTriangulated = 50;
  if (branch == 0) {
    int maxGood = nGood[0];
    for (int i = 1; i < 4; ++i) maxGood = nGood[i] > maxGood ? nGood[i] : maxGood;
    const int n09 = (int)(0.9 * N);
    const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
    int nsimilar = 0;
    for (int i = 0; i < 4; ++i) if (nGood[i] > 0.7 * maxGood) nsimilar++;
    int w = 3;
    for (int i = 3; i >= 0; --i) if (maxGood == nGood[i]) w = i;   // the if / else-if chain takes the first
    *winner = w;
    if (maxGood < nMinGood) return OSH_TWOVIEW_TOO_FEW_POINTS;
    if (nsimilar > 1) return OSH_TWOVIEW_NO_CLEAR_WINNER;
    return parallax[w] > minParallax ? OSH_TWOVIEW_ACCEPTED_F : OSH_TWOVIEW_LOW_PARALLAX;
  }
  int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
  float bestParallax = -1;
  for (int i = 0; i < 8; i++) {
    if (nGood[i] > bestGood) { secondBestGood = bestGood; bestGood = nGood[i]; bestSolutionIdx = i; bestParallax = parallax[i]; }
    else if (nGood[i] > secondBestGood) secondBestGood = nGood[i];
  }
  *winner = bestSolutionIdx;
  if (!(secondBestGood < 0.75 * bestGood)) return OSH_TWOVIEW_NO_CLEAR_WINNER;
  if (!(bestGood > minTriangulated && bestGood > 0.9 * N)) return OSH_TWOVIEW_TOO_FEW_POINTS;
  if (!(bestParallax >= minParallax)) return OSH_TWOVIEW_LOW_PARALLAX;
  return OSH_TWOVIEW_ACCEPTED_H;
}
OSH_KB8_HD void tv_head_clear(TvHead& h) {
  h.status = OSH_TWOVIEW_NO_MODEL; h.best_h = h.best_f = -1; h.branch = -1; h.n_inliers = 0; h.n_hyp = 0; h.winner = -1; h.pad = 0;
  for (int k = 0; k < 12; ++k) h.T21[k] = 0.f;
  h.sh = h.sf = 0.f;
  for (int k = 0; k < 9; ++k) h.H21[k] = h.F21[k] = 0.f;
  for (int i = 0; i < 8; ++i) {
    h.n_good[i] = 0; h.parallax[i] = 0.f;
    for (int k = 0; k < 9; ++k) h.R[i][k] = 0.f;
    for (int k = 0; k < 3; ++k) h.t[i][k] = 0.f;
  }
}
// :112-128 once both winners are known: the branch; the motion hypotheses follow from it
OSH_KB8_HD void tv_choose_branch(TvHead& h) {
#pragma clang fp contract(off)
  if (h.sh + h.sf == 0.f) { h.status = OSH_TWOVIEW_NO_MODEL; h.branch = -1; return; }
  const float RH = h.sh / (h.sh + h.sf);
  h.branch = (double)RH > 0.50 ? 1 : 0;
}
OSH_KB8_HD void tv_motion(const float* K, TvHead& h) {
  if (h.branch == 1) {
    if (tv_motion_h(h.H21, K, h.R, h.t)) h.n_hyp = 8;
    else { h.n_hyp = 0; h.status = OSH_TWOVIEW_H_DEGENERATE; }
  } else {
    tv_motion_f(h.F21, K, h.R, h.t);
    h.n_hyp = 4;
  }
}
OSH_KB8_HD void tv_finish(TvHead& h) {
  if (h.n_hyp == 0) return;   // no model, or H degenerate: the status stands
  int winner = -1;
  h.status = tv_decide(h.branch, h.n_inliers, h.n_good, h.parallax, &winner);
  h.winner = winner;
  if (winner >= 0) {
    for (int k = 0; k < 9; ++k) h.T21[k] = h.R[winner][k];
    for (int k = 0; k < 3; ++k) h.T21[9 + k] = h.t[winner][k];
  }
}

}  // namespace osh

// ---------------------------------------------------------------------------------------------------- the host build
#include <algorithm>
#include <cstring>
#include <vector>
namespace osh {

inline void tv_fill_problem(TvProblem& d, const osh_two_view_problem& p, int base_m, int base_h) {
  for (int k = 0; k < 9; ++k) { d.K[k] = p.K[k]; d.T1[k] = p.T1[k]; d.T2[k] = p.T2[k]; }
  d.sigma = p.sigma; d.n_iter = p.n_iterations; d.n_matches = p.n_matches; d.base_m = base_m; d.base_h = base_h;
}
// The head and the per-hypothesis debug arrays of a result
inline void tv_write_head(const osh_two_view_result& r, const TvHead& h) {
  if (r.status) *r.status = h.status;
  if (r.T21) std::memcpy(r.T21, h.T21, sizeof(h.T21));
  if (r.sh) *r.sh = h.sh;
  if (r.sf) *r.sf = h.sf;
  if (r.H21) std::memcpy(r.H21, h.H21, sizeof(h.H21));
  if (r.F21) std::memcpy(r.F21, h.F21, sizeof(h.F21));
  if (r.best_h) *r.best_h = h.best_h;
  if (r.best_f) *r.best_f = h.best_f;
  if (r.info) { r.info[0] = h.branch; r.info[1] = h.n_inliers; r.info[2] = h.n_hyp; r.info[3] = h.winner; }
  if (r.n_good) std::memcpy(r.n_good, h.n_good, sizeof(h.n_good));
  if (r.parallax) std::memcpy(r.parallax, h.parallax, sizeof(h.parallax));
  if (r.debug_R) std::memcpy(r.debug_R, h.R, sizeof(h.R));
  if (r.debug_t) std::memcpy(r.debug_t, h.t, sizeof(h.t));
}

// One problem (valid by the rules of osh_orb_two_view_reconstruct, any size) on one thread, every result word written.
inline void tv_reconstruct_host(const osh_two_view_problem& p, const osh_two_view_result& r) {
  const int n = p.n_matches, iters = p.n_iterations;
  TvHead h;
  tv_head_clear(h);
  const float invSigmaSquare = tv_inv_sigma_square(p.sigma);
  float T2inv[9], T2t[9];
  tv_inverse3(p.T2, T2inv);
  tv_transpose3(p.T2, T2t);
  float best_inv[9] = {0};
  for (int model = 0; model < 2; ++model) {
    float best_score = 0.f;
    int best = -1;
    for (int it = 0; it < iters; ++it) {
      float A[kTvRows][9], hv[9], Mn[9], M[9], Minv[9];
      for (int row = 0; row < kTvRows; ++row) {
        const int j = model == 0 ? row / 2 : (row < 8 ? row : 0);
        const int m = p.sets[8 * (size_t)it + j];
        tv_system_row(model, row, p.pn1[2 * m], p.pn1[2 * m + 1], p.pn2[2 * m], p.pn2[2 * m + 1], A[row]);
      }
      tv_null9(A, hv);
      tv_model(model, hv, model == 0 ? T2inv : T2t, p.T1, Mn, M, Minv);
      float score = 0.f;
      for (int i = 0; i < n; ++i) {
        float t1, t2;
        tv_check(model, M, Minv, invSigmaSquare, p.pt1[2 * i], p.pt1[2 * i + 1], p.pt2[2 * i], p.pt2[2 * i + 1], t1, t2);
        score = score + t1;
        score = score + t2;
      }
      const size_t g = (size_t)model * iters + it;
      if (r.debug_model_n) std::memcpy(r.debug_model_n + 9 * g, Mn, 36);
      if (r.debug_model) std::memcpy(r.debug_model + 9 * g, M, 36);
      if (r.debug_score) r.debug_score[g] = score;
      if (score > best_score) {
        best_score = score; best = it;
        std::memcpy(model == 0 ? h.H21 : h.F21, M, 36);
        if (model == 0) std::memcpy(best_inv, Minv, 36);
      }
    }
    if (model == 0) { h.sh = best_score; h.best_h = best; } else { h.sf = best_score; h.best_f = best; }
  }
  tv_choose_branch(h);
  std::vector<unsigned char> inl((size_t)n, 0);
  if (h.branch >= 0) {
    for (int i = 0; i < n; ++i) {
      float t1, t2;
      inl[i] = tv_check(h.branch == 1 ? 0 : 1, h.branch == 1 ? h.H21 : h.F21, best_inv, invSigmaSquare, p.pt1[2 * i], p.pt1[2 * i + 1], p.pt2[2 * i],
                        p.pt2[2 * i + 1], t1, t2) ? 1 : 0;
      h.n_inliers += inl[i];
    }
    tv_motion(p.K, h);
  }
  std::vector<float> x3d((size_t)8 * n * 3, 0.f);
  std::vector<unsigned char> code((size_t)8 * n, 0);
  const float th2 = tv_th2(p.sigma);
  for (int hyp = 0; hyp < h.n_hyp; ++hyp) {
    TvCamera2 c;
    tv_camera2(p.K, h.R[hyp], h.t[hyp], c);
    std::vector<unsigned> keys;
    for (int i = 0; i < n; ++i) {
      if (!inl[i]) continue;
      float cosp = 0.f;
      const size_t g = (size_t)hyp * n + i;
      code[g] = (unsigned char)tv_check_rt(p.K, h.R[hyp], h.t[hyp], c, th2, p.pt1[2 * i], p.pt1[2 * i + 1], p.pt2[2 * i], p.pt2[2 * i + 1], &x3d[3 * g], cosp);
      if (code[g]) keys.push_back(tv_cos_key(cosp));
    }
    h.n_good[hyp] = (int)keys.size();
    if (!keys.empty()) {
      std::sort(keys.begin(), keys.end());
      h.parallax[hyp] = tv_parallax(tv_key_cos(keys[std::min<size_t>(50, keys.size() - 1)]));
    }
  }
  tv_finish(h);
  tv_write_head(r, h);
  for (int i = 0; i < n; ++i) {
    const size_t g = (size_t)(h.winner < 0 ? 0 : h.winner) * n + i;
    const bool has = h.winner >= 0 && code[g];
    if (r.inlier) r.inlier[i] = inl[i];
    if (r.triangulated) r.triangulated[i] = h.winner >= 0 && code[g] == 2;
    if (r.x3d) for (int k = 0; k < 3; ++k) r.x3d[3 * (size_t)i + k] = has ? x3d[3 * g + k] : 0.f;
  }
}

}  // namespace osh
