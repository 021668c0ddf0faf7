// pgo4_se3.h -- the algebra of the 4-DoF pose graph (Optimizer::OptimizeEssentialGraph4DoF) restated for host and device:
// ImuCamPose::UpdateW (src/G2oTypes.cc:222-256) as VertexPose4DoF::oplusImpl drives it (include/G2oTypes.h:155-189),
// ExpSO3 / LogSO3 / NormalizeRotation (src/G2oTypes.cc:782-813, include/G2oTypes.h:67-71) and Edge4DoF::computeError
// (include/G2oTypes.h:817-845).  Matrices are 3x3 row-major; every product sums its terms left to right.
//
// NormalizeRotation is JacobiSVD's U V^T in the reference; here it is the same orthogonal polar factor by Newton iteration,
// as liba_math.h computes it.  liba_math.h is device-only and built with FMA contraction, so the functions are restated.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// No FMA contraction here: the central differences of the numeric Jacobians (delta 1e-9) amplify every rounding difference
// by 5e8, and the tests compare them with a restatement that rounds each operation.
#pragma clang fp contract(off)

namespace osh {
namespace pgo4 {

// The mutable part of one vertex: what g2o's push / pop saves and restores.
struct State {
  double DR[9];    // accumulated yaw rotation
  double Rwb[9];
  double twb[3];
  double Rcw[9];   // camera pose: the raw pose until the first update, then Rcb Rwb^T, Rcb (-Rwb^T twb) + tcb
  double tcw[3];
  int its;         // updates since the last normalisation of DR
};
constexpr int kStateDoubles = 34;   // DR Rwb twb Rcw tcw its
constexpr int kConstDoubles = 21;   // Rwb0 Rcb tcb

// The fixed part: Rwb0 (the initial Rwb) and the IMU-to-camera transform.
struct Const {
  double Rwb0[9];
  double Rcb[9];
  double tcb[3];
};

__host__ __device__ inline State state_load(const double* p) {
  State s;
  for (int k = 0; k < 9; ++k) s.DR[k] = p[k];
  for (int k = 0; k < 9; ++k) s.Rwb[k] = p[9 + k];
  for (int k = 0; k < 3; ++k) s.twb[k] = p[18 + k];
  for (int k = 0; k < 9; ++k) s.Rcw[k] = p[21 + k];
  for (int k = 0; k < 3; ++k) s.tcw[k] = p[30 + k];
  s.its = (int)p[33];
  return s;
}
__host__ __device__ inline void state_store(const State& s, double* p) {
  for (int k = 0; k < 9; ++k) p[k] = s.DR[k];
  for (int k = 0; k < 9; ++k) p[9 + k] = s.Rwb[k];
  for (int k = 0; k < 3; ++k) p[18 + k] = s.twb[k];
  for (int k = 0; k < 9; ++k) p[21 + k] = s.Rcw[k];
  for (int k = 0; k < 3; ++k) p[30 + k] = s.tcw[k];
  p[33] = (double)s.its;
}
__host__ __device__ inline Const const_load(const double* p) {
  Const c;
  for (int k = 0; k < 9; ++k) c.Rwb0[k] = p[k];
  for (int k = 0; k < 9; ++k) c.Rcb[k] = p[9 + k];
  for (int k = 0; k < 3; ++k) c.tcb[k] = p[18 + k];
  return c;
}

__host__ __device__ inline void m3_mul(const double* A, const double* B, double* C) {   // C = A B
  double T[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
  for (int i = 0; i < 9; ++i) C[i] = T[i];
}
__host__ __device__ inline void m3_mul_bt(const double* A, const double* B, double* C) {   // C = A B^T
  double T[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1] + A[i * 3 + 2] * B[j * 3 + 2];
  for (int i = 0; i < 9; ++i) C[i] = T[i];
}
__host__ __device__ inline void m3_vec(const double* A, const double* v, double* o) {   // o = A v
  const double t0 = A[0] * v[0] + A[1] * v[1] + A[2] * v[2], t1 = A[3] * v[0] + A[4] * v[1] + A[5] * v[2];
  const double t2 = A[6] * v[0] + A[7] * v[1] + A[8] * v[2];
  o[0] = t0; o[1] = t1; o[2] = t2;
}
__host__ __device__ inline void m3_tvec(const double* A, const double* v, double* o) {   // o = A^T v
  const double t0 = A[0] * v[0] + A[3] * v[1] + A[6] * v[2], t1 = A[1] * v[0] + A[4] * v[1] + A[7] * v[2];
  const double t2 = A[2] * v[0] + A[5] * v[1] + A[8] * v[2];
  o[0] = t0; o[1] = t1; o[2] = t2;
}

// NormalizeRotation: the orthogonal polar factor, R <- (R + R^-T) / 2 until no entry moves by 1e-16
__host__ __device__ inline void normalize_rotation(double* R) {
  for (int it = 0; it < 12; ++it) {
    const double c00 = R[4] * R[8] - R[5] * R[7], c10 = R[5] * R[6] - R[3] * R[8], c20 = R[3] * R[7] - R[4] * R[6];
    const double id = 1.0 / (R[0] * c00 + R[1] * c10 + R[2] * c20);
    const double Ri[9] = {c00 * id, (R[2] * R[7] - R[1] * R[8]) * id, (R[1] * R[5] - R[2] * R[4]) * id,
                          c10 * id, (R[0] * R[8] - R[2] * R[6]) * id, (R[2] * R[3] - R[0] * R[5]) * id,
                          c20 * id, (R[1] * R[6] - R[0] * R[7]) * id, (R[0] * R[4] - R[1] * R[3]) * id};
    double d = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double nv = 0.5 * (R[i * 3 + j] + Ri[j * 3 + i]);
        d = fmax(d, fabs(nv - R[i * 3 + j]));
        R[i * 3 + j] = nv;
      }
    if (d < 1e-16) break;
  }
}

// ExpSO3(x, y, z): I + W + 0.5 W^2 below 1e-5, else I + W sin(d) / d + W^2 (1 - cos(d)) / d^2; then NormalizeRotation
__host__ __device__ inline void exp_so3(double x, double y, double z, double* R) {
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  const double W[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
  double W2[9];
  m3_mul(W, W, W2);
  if (d < 1e-5) {
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + W[i]) + 0.5 * W2[i];
  } else {
    const double s = sin(d), c = 1.0 - cos(d);
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + (W[i] * s) / d) + (W2[i] * c) / d2;
  }
  normalize_rotation(R);
}

// LogSO3 (src/G2oTypes.cc:800-813)
__host__ __device__ inline void log_so3(const double* R, double* w) {
  const double tr = R[0] + R[4] + R[8];
  w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
  const double costheta = (tr - 1.0) * 0.5;
  if (costheta > 1 || costheta < -1) return;
  const double theta = acos(costheta), s = sin(theta);
  if (fabs(s) < 1e-5) return;
  for (int k = 0; k < 3; ++k) w[k] = (theta * w[k]) / s;
}

// VertexPose4DoF::oplusImpl: u = (yaw, tx, ty, tz) -> UpdateW(0, 0, yaw, tx, ty, tz)
__host__ __device__ inline void update_w(State& s, const Const& c, const double* u) {
  double dR[9];
  exp_so3(0.0, 0.0, u[0], dR);
  m3_mul(dR, s.DR, s.DR);
  m3_mul(s.DR, c.Rwb0, s.Rwb);
  for (int k = 0; k < 3; ++k) s.twb[k] += u[1 + k];
  s.its++;
  if (s.its >= 5) {
    s.DR[2] = 0.0; s.DR[5] = 0.0; s.DR[6] = 0.0; s.DR[7] = 0.0;
    normalize_rotation(s.DR);
    s.its = 0;
  }
  double Rbw[9], tbw[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rbw[i * 3 + j] = s.Rwb[j * 3 + i];
  m3_vec(Rbw, s.twb, tbw);
  for (int k = 0; k < 3; ++k) tbw[k] = -tbw[k];
  m3_mul(c.Rcb, Rbw, s.Rcw);
  double t[3];
  m3_vec(c.Rcb, tbw, t);
  for (int k = 0; k < 3; ++k) s.tcw[k] = t[k] + c.tcb[k];
}

// Edge4DoF::computeError: [ LogSO3(Rcw_i Rcw_j^T dR^T) ; Rcw_i (-Rcw_j^T tcw_j) + tcw_i - dt ]
__host__ __device__ inline void edge_error(const double* dR, const double* dt, const double* Rcwi, const double* tcwi, const double* Rcwj,
                                           const double* tcwj, double* e) {
  double A[9], B[9];
  m3_mul_bt(Rcwi, Rcwj, A);
  m3_mul_bt(A, dR, B);
  log_so3(B, e);
  double v[3], r[3];
  m3_tvec(Rcwj, tcwj, v);
  for (int k = 0; k < 3; ++k) v[k] = -v[k];
  m3_vec(Rcwi, v, r);
  for (int k = 0; k < 3; ++k) e[3 + k] = (r[k] + tcwi[k]) - dt[k];
}

}  // namespace pgo4
}  // namespace osh
