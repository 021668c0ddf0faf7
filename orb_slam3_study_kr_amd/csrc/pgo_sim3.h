// pgo_sim3.h -- g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) restated for the device, with the same branches and the same
// operation order: exp from a 7-vector omega, upsilon, sigma (:70-146), map (:144), log (:148-231), inverse (:233),
// product (:266).  Quaternions are stored x y z w as g2o::Sim3::operator[] exposes them; Quaterniond(Matrix3d) and
// toRotationMatrix() follow Eigen (Geometry/Quaternion.h), the 3x3 solve of log() is a partial-pivot LU as Eigen's lu().
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// No FMA contraction here: the central differences of the numeric Jacobians (delta 1e-9) amplify every rounding difference
// by 5e8, and the tests compare them with a restatement that rounds each operation.
#pragma clang fp contract(off)

namespace osh {
namespace pgo {

struct Sim3 {
  double q[4];   // x y z w
  double t[3];
  double s;
};

__host__ __device__ inline Sim3 sim3_load(const double* p) {
  Sim3 r;
  for (int k = 0; k < 4; ++k) r.q[k] = p[k];
  for (int k = 0; k < 3; ++k) r.t[k] = p[4 + k];
  r.s = p[7];
  return r;
}
__host__ __device__ inline void sim3_store(const Sim3& a, double* p) {
  for (int k = 0; k < 4; ++k) p[k] = a.q[k];
  for (int k = 0; k < 3; ++k) p[4 + k] = a.t[k];
  p[7] = a.s;
}

// Eigen: q * v = v + w uv + vec x uv with uv = 2 (vec x v)
__host__ __device__ inline void quat_rotate(const double* q, const double* v, double* o) {
  double uv0 = q[1] * v[2] - q[2] * v[1], uv1 = q[2] * v[0] - q[0] * v[2], uv2 = q[0] * v[1] - q[1] * v[0];
  uv0 += uv0; uv1 += uv1; uv2 += uv2;
  o[0] = v[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1);
  o[1] = v[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2);
  o[2] = v[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0);
}

__host__ __device__ inline void quat_mul(const double* a, const double* b, double* o) {
  const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
  o[3] = aw * bw - ax * bx - ay * by - az * bz;
  o[0] = aw * bx + ax * bw + ay * bz - az * by;
  o[1] = aw * by + ay * bw + az * bx - ax * bz;
  o[2] = aw * bz + az * bw + ax * by - ay * bx;
}

// Quaternion::toRotationMatrix
__host__ __device__ inline void quat_to_R(const double* q, double R[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// Quaterniond(const Matrix3d&) (no normalisation)
__host__ __device__ inline void R_to_quat(const double R[9], double* q) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    double t = sqrt(tr + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
}

__host__ __device__ inline void skew(const double* w, double O[9]) {
  O[0] = 0; O[1] = -w[2]; O[2] = w[1];
  O[3] = w[2]; O[4] = 0; O[5] = -w[0];
  O[6] = -w[1]; O[7] = w[0]; O[8] = 0;
}
__host__ __device__ inline void mat3_mul(const double* a, const double* b, double* o) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3] * b[c] + a[r * 3 + 1] * b[3 + c] + a[r * 3 + 2] * b[6 + c];
}

// Sim3(const Vector7d& update)
__host__ __device__ inline Sim3 sim3_exp(const double* u) {
  const double omega[3] = {u[0], u[1], u[2]}, upsilon[3] = {u[3], u[4], u[5]};
  const double sigma = u[6];
  const double theta = sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
  double Om[9], Om2[9], R[9];
  skew(omega, Om);
  Sim3 r;
  r.s = exp(sigma);
  mat3_mul(Om, Om, Om2);
  const double eps = 0.00001;
  double A, B, C;
  bool small_theta = theta < eps;
  if (fabs(sigma) < eps) {
    C = 1;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (r.s - 1) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * r.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * r.s) / (sigma2 * sigma);
    } else {
      const double a = r.s * sin(theta), b = r.s * cos(theta);
      const double theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  if (small_theta) {
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0 ? 1.0 : 0.0) + Om[k] + Om2[k];   // I + Omega + Omega*Omega
  } else {
    const double f1 = sin(theta) / theta, f2 = (1 - cos(theta)) / (theta * theta);
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0 ? 1.0 : 0.0) + f1 * Om[k] + f2 * Om2[k];
  }
  R_to_quat(R, r.q);
  double W[9];
  for (int k = 0; k < 9; ++k) W[k] = A * Om[k] + B * Om2[k] + (k % 4 == 0 ? C : 0.0);
  for (int k = 0; k < 3; ++k) r.t[k] = W[k * 3] * upsilon[0] + W[k * 3 + 1] * upsilon[1] + W[k * 3 + 2] * upsilon[2];
  return r;
}

// W.lu().solve(t): partial pivoting by rows
__host__ __device__ inline void solve3_lu(const double* Win, const double* t, double* x) {
  double a[9], b[3] = {t[0], t[1], t[2]};
  for (int k = 0; k < 9; ++k) a[k] = Win[k];
  for (int k = 0; k < 3; ++k) {
    int p = k;
    double best = fabs(a[k * 3 + k]);
    for (int i = k + 1; i < 3; ++i) if (fabs(a[i * 3 + k]) > best) { best = fabs(a[i * 3 + k]); p = i; }
    if (p != k) {
      for (int c = 0; c < 3; ++c) { const double tmp = a[k * 3 + c]; a[k * 3 + c] = a[p * 3 + c]; a[p * 3 + c] = tmp; }
      const double tmp = b[k]; b[k] = b[p]; b[p] = tmp;
    }
    for (int i = k + 1; i < 3; ++i) {
      const double l = a[i * 3 + k] / a[k * 3 + k];
      for (int c = k + 1; c < 3; ++c) a[i * 3 + c] -= l * a[k * 3 + c];
      b[i] -= l * b[k];
    }
  }
  for (int k = 2; k >= 0; --k) {
    double s = b[k];
    for (int c = k + 1; c < 3; ++c) s -= a[k * 3 + c] * x[c];
    x[k] = s / a[k * 3 + k];
  }
}

__host__ __device__ inline void sim3_log(const Sim3& S, double* res) {
  const double sigma = log(S.s);
  double R[9], Om[9], Om2[9], omega[3];
  quat_to_R(S.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR (se3_ops.hpp:40-47)
  const double eps = 0.00001;
  double A, B, C;
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta = acos(d), theta2 = theta * theta;
      const double f = theta / (2 * sqrt(1 - d * d));
      for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
      A = ((sigma - 1) * S.s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta = acos(d);
      const double f = theta / (2 * sqrt(1 - d * d));
      for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
      const double theta2 = theta * theta, a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  skew(omega, Om);
  mat3_mul(Om, Om, Om2);
  double W[9];
  for (int k = 0; k < 9; ++k) W[k] = A * Om[k] + B * Om2[k] + (k % 4 == 0 ? C : 0.0);
  double ups[3];
  solve3_lu(W, S.t, ups);
  for (int k = 0; k < 3; ++k) { res[k] = omega[k]; res[3 + k] = ups[k]; }
  res[6] = sigma;
}

__host__ __device__ inline Sim3 sim3_inverse(const Sim3& a) {
  Sim3 r;
  r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
  const double f = -1. / a.s;
  const double mt[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
  quat_rotate(r.q, mt, r.t);
  r.s = 1. / a.s;
  return r;
}

__host__ __device__ inline Sim3 sim3_mul(const Sim3& a, const Sim3& b) {
  Sim3 r;
  quat_mul(a.q, b.q, r.q);
  double rt[3];
  quat_rotate(a.q, b.t, rt);
  for (int k = 0; k < 3; ++k) r.t[k] = a.s * rt[k] + a.t[k];
  r.s = a.s * b.s;
  return r;
}

__host__ __device__ inline void sim3_map(const Sim3& a, const double* p, double* o) {
  double rp[3];
  quat_rotate(a.q, p, rp);
  for (int k = 0; k < 3; ++k) o[k] = a.s * rp[k] + a.t[k];
}

// EdgeSim3::computeError (types_seven_dof_expmap.h:99-112): log(Sji * Si * Sj^-1)
__host__ __device__ inline void edge_error(const Sim3& meas, const Sim3& Si, const Sim3& Sj, double* e) {
  sim3_log(sim3_mul(sim3_mul(meas, Si), sim3_inverse(Sj)), e);
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): estimate <- Sim3(update) * estimate, update[6] = 0 with _fix_scale
__host__ __device__ inline Sim3 vertex_oplus(const Sim3& est, const double* upd, bool fix_scale) {
  double u[7];
  for (int k = 0; k < 7; ++k) u[k] = upd[k];
  if (fix_scale) u[6] = 0;
  return sim3_mul(sim3_exp(u), est);
}

}  // namespace pgo
}  // namespace osh
