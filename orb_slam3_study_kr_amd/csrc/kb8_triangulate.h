// kb8_triangulate.h -- KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:306-375) with unproject (:116-143),
// project(Vector3f) (:67-84) and Triangulate (:394-406), for one keypoint pair.  Device code of fisheye_stereo_device.hip; plain C++
// as well, so the test library can run the same statements on the host.
//
// Float32 steps are single IEEE operations in the reference's order with contraction off; Eigen's three-term reductions (dot, norm,
// matrix * vector) are a0 + (a1 + a2) as in k_frustum (orb_device.hip); sqrtf, tan, atan2f, cos and sin are the FP64 function rounded
// once.  The one deviation: the right singular vector of A's smallest singular value comes from a one-sided Jacobi method in FP64
// with a fixed number of sweeps (no data-dependent loop) instead of Eigen's float JacobiSVD, and x3D is rounded to float32 once,
// after the division by w.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OSH_KB8_HD __host__ __device__ inline
#else
#define OSH_KB8_HD inline
#endif

namespace osh {

struct Kb8Rig {
  float cam1[8], cam2[8];   // fx fy cx cy k1 k2 k3 k4
  float prec1, prec2;       // KannalaBrandt8::precision
  float R12[9], t12[3];     // row-major
};

constexpr int kKb8Sweeps = 8;   // one-sided Jacobi sweeps over the six column pairs of a 4x4 matrix (convergence is quadratic); with 8 the
                                // host build equals LAPACK's FP64 SVD in every float32 bit of x3D on the committed test cases

OSH_KB8_HD float kb8_sum3(float a0, float a1, float a2) {
#pragma clang fp contract(off)
  return a0 + (a1 + a2);
}
OSH_KB8_HD float kb8_sqrt(float x) { return (float)sqrt((double)x); }   // correctly rounded: 53 >= 2 * 24 + 2

// :116-143
OSH_KB8_HD void kb8_unproject(const float* cam, float precision, float x, float y, float r[3]) {
#pragma clang fp contract(off)
  const float pwx = (x - cam[2]) / cam[0], pwy = (y - cam[3]) / cam[1];
  float scale = 1.f;
  float theta_d = kb8_sqrt(pwx * pwx + pwy * pwy);
  const float half_pi = (float)(3.1415926535897932384626433832795 / 2.0);   // CV_PI / 2.f, a double, narrowed by fminf / fmaxf
  theta_d = fminf(fmaxf(-half_pi, theta_d), half_pi);
  if ((double)theta_d > 1e-8) {
    float theta = theta_d;
    for (int j = 0; j < 10; j++) {
      const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
      const float k0_theta2 = cam[4] * theta2, k1_theta4 = cam[5] * theta4;
      const float k2_theta6 = cam[6] * theta6, k3_theta8 = cam[7] * theta8;
      const float theta_fix = (theta * (1.f + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                              (1.f + 3.f * k0_theta2 + 5.f * k1_theta4 + 7.f * k2_theta6 + 9.f * k3_theta8);
      theta = theta - theta_fix;
      if (fabsf(theta_fix) < precision) break;
    }
    scale = (float)tan((double)theta) / theta_d;
  }
  r[0] = pwx * scale; r[1] = pwy * scale; r[2] = 1.f;
}

// :67-84
OSH_KB8_HD void kb8_project(const float* cam, const float v[3], float uv[2]) {
#pragma clang fp contract(off)
  const float x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
  const float theta = (float)atan2((double)kb8_sqrt(x2_plus_y2), (double)v[2]);
  const float psi = (float)atan2((double)v[1], (double)v[0]);
  const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
  const float r = theta + cam[4] * theta3 + cam[5] * theta5 + cam[6] * theta7 + cam[7] * theta9;
  uv[0] = cam[0] * r * (float)cos((double)psi) + cam[2];
  uv[1] = cam[1] * r * (float)sin((double)psi) + cam[3];
}

// One rotation of the one-sided Jacobi method: makes columns P and Q of a orthogonal and applies the same rotation to V.
template <int P, int Q>
OSH_KB8_HD void kb8_rotate(double (&a)[4][4], double (&v)[4][4]) {
#pragma clang fp contract(off)
  double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { alpha += a[i][P] * a[i][P]; beta += a[i][Q] * a[i][Q]; gamma += a[i][P] * a[i][Q]; }
  const double zeta = (beta - alpha) / (2.0 * gamma);
  double t = (zeta < 0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  if (gamma == 0.0 || !(t == t)) t = 0.0;             // orthogonal already (or 0 / 0, inf / inf): no rotation
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double ap = a[i][P], aq = a[i][Q], vp = v[i][P], vq = v[i][Q];
    a[i][P] = c * ap - s * aq; a[i][Q] = s * ap + c * aq;
    v[i][P] = c * vp - s * vq; v[i][Q] = s * vp + c * vq;
  }
}

// :394-406: h = the right singular vector of A's smallest singular value, homogeneous (newpoint_triangulate.h tests h[3] == 0)
OSH_KB8_HD void kb8_null_vector_h(const float A[4][4], double h[4]) {
#pragma clang fp contract(off)
  double a[4][4], v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[i][j] = (double)A[i][j]; v[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < kKb8Sweeps; ++sweep) {
    kb8_rotate<0, 1>(a, v); kb8_rotate<0, 2>(a, v); kb8_rotate<0, 3>(a, v);
    kb8_rotate<1, 2>(a, v); kb8_rotate<1, 3>(a, v); kb8_rotate<2, 3>(a, v);
  }
  double best = 0;
  h[0] = h[1] = h[2] = h[3] = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) n += a[i][j] * a[i][j];
    if (j == 0 || n < best) {
      best = n;
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = v[i][j];
    }
  }
}

// x3D = head(3) / w of it, rounded to float32 once
OSH_KB8_HD void kb8_null_vector(const float A[4][4], float x3D[3]) {
#pragma clang fp contract(off)
  double h[4];
  kb8_null_vector_h(A, h);
  x3D[0] = (float)(h[0] / h[3]); x3D[1] = (float)(h[1] / h[3]); x3D[2] = (float)(h[2] / h[3]);
}

// :306-375.  Returns z1 or -1 .. -5; p3d = x3D when the pair passes every test, else 0 0 0; *cos_parallax = cosParallaxRays.
OSH_KB8_HD float kb8_triangulate_match(const Kb8Rig& g, float x1, float y1, float x2, float y2, float sigmaLevel, float unc, float p3d[3],
                                       float* cos_parallax) {
#pragma clang fp contract(off)
  p3d[0] = p3d[1] = p3d[2] = 0.f;
  float r1[3], r2[3], r21[3];
  kb8_unproject(g.cam1, g.prec1, x1, y1, r1);
  kb8_unproject(g.cam2, g.prec2, x2, y2, r2);
#pragma unroll
  for (int i = 0; i < 3; ++i) r21[i] = kb8_sum3(g.R12[3 * i] * r2[0], g.R12[3 * i + 1] * r2[1], g.R12[3 * i + 2] * r2[2]);
  const float dot = kb8_sum3(r1[0] * r21[0], r1[1] * r21[1], r1[2] * r21[2]);
  const float n1 = kb8_sqrt(kb8_sum3(r1[0] * r1[0], r1[1] * r1[1], r1[2] * r1[2]));
  const float n21 = kb8_sqrt(kb8_sum3(r21[0] * r21[0], r21[1] * r21[1], r21[2] * r21[2]));
  const float cosParallaxRays = dot / (n1 * n21);
  *cos_parallax = cosParallaxRays;
  if ((double)cosParallaxRays > 0.9998) return -1.f;
  // Tcw1 = [I | 0], Tcw2 = [R21 | -R21 * t12]
  float T2[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) T2[i][j] = g.R12[3 * j + i];
    T2[i][3] = -kb8_sum3(T2[i][0] * g.t12[0], T2[i][1] * g.t12[1], T2[i][2] * g.t12[2]);
  }
  float A[4][4] = {{-1.f, 0.f, r1[0], 0.f}, {0.f, -1.f, r1[1], 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // p * row(2) - row(0 / 1) of [I | 0]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A[2][j] = r2[0] * T2[2][j] - T2[0][j];
    A[3][j] = r2[1] * T2[2][j] - T2[1][j];
  }
  float x3D[3];
  kb8_null_vector(A, x3D);
  const float z1 = x3D[2];
  if (z1 <= 0) return -2.f;
  const float z2 = kb8_sum3(T2[2][0] * x3D[0], T2[2][1] * x3D[1], T2[2][2] * x3D[2]) + T2[2][3];
  if (z2 <= 0) return -3.f;
  float uv1[2], uv2[2], x3D2[3];
  kb8_project(g.cam1, x3D, uv1);
  const float errX1 = uv1[0] - x1, errY1 = uv1[1] - y1;
  if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaLevel) return -4.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) x3D2[i] = kb8_sum3(T2[i][0] * x3D[0], T2[i][1] * x3D[1], T2[i][2] * x3D[2]) + T2[i][3];
  kb8_project(g.cam2, x3D2, uv2);
  const float errX2 = uv2[0] - x2, errY2 = uv2[1] - y2;
  if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)unc) return -5.f;
  p3d[0] = x3D[0]; p3d[1] = x3D[1]; p3d[2] = x3D[2];
  return z1;
}

}  // namespace osh
