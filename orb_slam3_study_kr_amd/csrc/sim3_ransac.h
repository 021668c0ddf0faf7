// sim3_ransac.h -- Sim3Solver (src/Sim3Solver.cc), the Sim3 RANSAC of loop closing and map merging: ComputeSim3 (:311-412, Horn's
// closed form over a minimal set of 3 correspondences), CheckInliers / Project (:415-475) and the record bookkeeping of iterate
// (:167-210, :240-288) behind its minimal-set draw.  Device code of sim3_ransac_device.hip; plain C++ as well: s3r_solve_host at the
// end is the whole pipeline on one thread (the host build the test library, the make target sim3-ransac-check and the drop-in's
// fall-back run).
//
// Every statement is a single IEEE operation with contraction off.  What the reference's statements give:
//   * Centroids (:302-308): C = ((p0 + p1) + p2) / 3.f per coordinate, Pr.col(i) = P.col(i) - C, float32.
//   * M = Pr2 * Pr1^T (:328): M(i, j) = ((Pr2(i,0) * Pr1(j,0) + Pr2(i,1) * Pr1(j,1)) + Pr2(i,2) * Pr1(j,2)), float32, never fused.
//   * N (:335-349): the ten entries formed in double from the float entries of M, left to right, each rounded to float32 once (the
//     reference stores them in a Matrix4f).
//   * P3 = mR12i * Pr2 (:371) in float32, three-term sums left to right.  nom = sum(Pr1 .* P3) and den = sum(P3 .* P3) (:378-383):
//     float products accumulated in float in storage order (point after point, x y z), then widened; ms12i = (float)(nom / den), or
//     1.0f with bFixScale.  den == 0 gives an infinite or NaN scale: every comparison of CheckInliers is then false, 0 inliers.
//   * sR = ms12i * mR12i per entry; mt12i = O1 - sR * O2 (:391); sRinv = (float)(1.0 / (double)ms12i) * mR12i^T per entry (:405);
//     tinv = -(sRinv * mt12i) (:410); all float32, three-term sums left to right.
//   * Project (:461-475): P = ((r0 * x + r1 * y) + r2 * z) + t per row of [sR | t] in float32, then the camera's float project
//     (Pinhole: fx * x / z + cx; KannalaBrandt8: kb8_project of kb8_triangulate.h).  The two cameras may differ.
//   * CheckInliers (:415-439): err = dx * dx + dy * dy in float32; inlier when err1 < max1 && err2 < max2.  The thresholds arrive as
//     floats; the drop-in class fills them with the reference's truncation to size_t.
// What is defined here and not by the reference (Eigen is not available, so parity with it is unpinned):
//   * The eigenvector of the largest eigenvalue of the symmetric N: the cyclic two-sided Jacobi method in FP64 on the float32 entries,
//     kS3rSweeps sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), the rotation of a pair from jacobi_rotation (jacobi_rows.h) of
//     (a_pp, a_qq, a_pq) applied to both columns and both rows with jacobi_rotate_pair and to the columns of V; a pair with a_pq == 0
//     is not rotated.  (The one-sided method of jacobi_rows.h does not fit: N of three points has the eigenvalues +-(s1 + s2), +-(s1 - s2),
//     so its largest singular value is double.)  The eigenvalues are the diagonal; the largest wins, the first column on a tie.
//     The vector is divided by its norm and its sign set so that its real part is >= 0.  The reference runs Eigen's EigenSolver in float.
//   * mR12i is the rotation matrix of that unit quaternion (w, x, y, z), formed in FP64 and rounded to float32 once.  The reference goes
//     through atan2, an angle-axis vector divided by vec.norm() (0 for the identity) and Sophus::SO3f::exp.  Here (1,0,0,0) gives the
//     identity and no NaN.
//   * Records: iteration k is a record when count_k >= the running best, which starts at best_inliers_in (ties go to the later
//     iteration); it is a hit when it is a record and count_k > min_inliers.  The running best goes on across a hit.
// No loop here depends on a convergence test: every bound is fixed, a NaN input ends in 0 inliers.
#pragma once
#include "jacobi_rows.h"
#include "ransac_stage.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace osh {

constexpr int kS3rWave = 64;
constexpr int kS3rSweeps = 10;   // as kJacobiSweeps; with 10 the host build equals LAPACK's FP64 eigh in every float32 bit of R, t, s on the
                                 // well-conditioned test sets (tests/sim3_ransac_cases.py)

struct S3rProblem {
  int camera_type1, camera_type2;
  float cam1[8], cam2[8];
  int fix_scale, n, n_iter, min_inliers, best_in;
  int words;            // mask words of one iteration: 2 * ceil(n / 64)
  int base_p, base_h;   // offsets of the problem's correspondences and iterations in the arrays of the batch
  int base_w;           // offset of its iterations' mask words
};
struct S3rHead { int first_hit, n_records, best_iteration, best_count; };

// One hypothesis: R (row-major), t, s as the 13 floats of the interface, and what CheckInliers projects with
struct S3rTransform {
  float sR[9], t[3];         // mT12i
  float sRinv[9], tinv[3];   // mT21i
};

// ---------------------------------------------------------------------------------------------------- ComputeSim3 (:311-412)
template <int P, int Q>
OSH_KB8_HD void s3r_jacobi_pair(double (&a)[4][4], double (&v)[4][4]) {
#pragma clang fp contract(off)
  double c, s;
  jacobi_rotation(a[P][P], a[Q][Q], a[P][Q], c, s);
#pragma unroll
  for (int r = 0; r < 4; ++r) jacobi_rotate_pair(a[r][P], a[r][Q], c, s);
#pragma unroll
  for (int r = 0; r < 4; ++r) jacobi_rotate_pair(a[P][r], a[Q][r], c, s);
#pragma unroll
  for (int r = 0; r < 4; ++r) jacobi_rotate_pair(v[r][P], v[r][Q], c, s);
}
// The unit eigenvector (w, x, y, z) of the largest eigenvalue of the symmetric 4x4 matrix N (row-major), w >= 0
OSH_KB8_HD void s3r_top_eigenvector(const float* N, double q[4]) {
#pragma clang fp contract(off)
  double a[4][4], v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[i][j] = (double)N[4 * i + j]; v[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < kS3rSweeps; ++sweep) {
    s3r_jacobi_pair<0, 1>(a, v); s3r_jacobi_pair<0, 2>(a, v); s3r_jacobi_pair<0, 3>(a, v);
    s3r_jacobi_pair<1, 2>(a, v); s3r_jacobi_pair<1, 3>(a, v); s3r_jacobi_pair<2, 3>(a, v);
  }
  double best = a[0][0];
  q[0] = v[0][0]; q[1] = v[1][0]; q[2] = v[2][0]; q[3] = v[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (a[j][j] > best) { best = a[j][j]; q[0] = v[0][j]; q[1] = v[1][j]; q[2] = v[2][j]; q[3] = v[3][j]; }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sign = q[0] < 0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = sign * (q[k] / n);
}
// The rotation matrix of the unit quaternion (w, x, y, z), rounded to float32 once
OSH_KB8_HD void s3r_quaternion_rotation(const double q[4], float* R) {
#pragma clang fp contract(off)
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = (float)(1.0 - 2.0 * (yy + zz)); R[1] = (float)(2.0 * (xy - wz)); R[2] = (float)(2.0 * (xz + wy));
  R[3] = (float)(2.0 * (xy + wz)); R[4] = (float)(1.0 - 2.0 * (xx + zz)); R[5] = (float)(2.0 * (yz - wx));
  R[6] = (float)(2.0 * (xz - wy)); R[7] = (float)(2.0 * (yz + wx)); R[8] = (float)(1.0 - 2.0 * (xx + yy));
}
// :302-308.  P: three points, P[3 * k + i] coordinate i of point k; Pr the same layout
OSH_KB8_HD void s3r_centroid(const float* P, float* Pr, float* C) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float sum = (P[i] + P[3 + i]) + P[6 + i];
    C[i] = sum / 3.f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < 3; ++i) Pr[3 * k + i] = P[3 * k + i] - C[i];
}
// N (row-major 4x4) of the two centred sets (:328-349)
OSH_KB8_HD void s3r_horn_matrix(const float* Pr1, const float* Pr2, float* N) {
#pragma clang fp contract(off)
  float M[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = (Pr2[i] * Pr1[j] + Pr2[3 + i] * Pr1[3 + j]) + Pr2[6 + i] * Pr1[6 + j];
  const double m00 = (double)M[0][0], m01 = (double)M[0][1], m02 = (double)M[0][2], m10 = (double)M[1][0], m11 = (double)M[1][1],
               m12 = (double)M[1][2], m20 = (double)M[2][0], m21 = (double)M[2][1], m22 = (double)M[2][2];
  const float N11 = (float)(m00 + m11 + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10);
  const float N22 = (float)(m00 - m11 - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02);
  const float N33 = (float)(-m00 + m11 - m22), N34 = (float)(m12 + m21), N44 = (float)(-m00 - m11 + m22);
  N[0] = N11; N[1] = N12; N[2] = N13; N[3] = N14;
  N[4] = N12; N[5] = N22; N[6] = N23; N[7] = N24;
  N[8] = N13; N[9] = N23; N[10] = N33; N[11] = N34;
  N[12] = N14; N[13] = N24; N[14] = N34; N[15] = N44;
}
// mT12i and mT21i of R, t, s (:398-411)
OSH_KB8_HD void s3r_transforms(const float* R, const float* t, float s, S3rTransform& T) {
#pragma clang fp contract(off)
  const float sinv = (float)(1.0 / (double)s);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { T.sR[3 * i + j] = s * R[3 * i + j]; T.sRinv[3 * i + j] = sinv * R[3 * j + i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T.t[i] = t[i];
    T.tinv[i] = -((T.sRinv[3 * i] * t[0] + T.sRinv[3 * i + 1] * t[1]) + T.sRinv[3 * i + 2] * t[2]);
  }
}
// P1, P2: the three members of the minimal set in camera 1 and camera 2 (P[3 * k + i]); T13 = R (row-major), t, s
OSH_KB8_HD void s3r_compute_sim3(const float* P1, const float* P2, bool fix_scale, float* T13) {
#pragma clang fp contract(off)
  float Pr1[9], Pr2[9], O1[3], O2[3], N[16];
  s3r_centroid(P1, Pr1, O1);
  s3r_centroid(P2, Pr2, O2);
  s3r_horn_matrix(Pr1, Pr2, N);
  double q[4];
  s3r_top_eigenvector(N, q);
  float* R = T13;
  s3r_quaternion_rotation(q, R);
  float s = 1.0f;
  if (!fix_scale) {
    float nom = 0.f, den = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float p3 = (R[3 * i] * Pr2[3 * k] + R[3 * i + 1] * Pr2[3 * k + 1]) + R[3 * i + 2] * Pr2[3 * k + 2];
        nom = nom + Pr1[3 * k + i] * p3;
        den = den + p3 * p3;
      }
    s = (float)((double)nom / (double)den);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float a = s * R[3 * i], b = s * R[3 * i + 1], c = s * R[3 * i + 2];
    T13[9 + i] = O1[i] - ((a * O2[0] + b * O2[1]) + c * O2[2]);
  }
  T13[12] = s;
}

// ---------------------------------------------------------------------------------------------------- CheckInliers (:415-475)
OSH_KB8_HD void s3r_project(int camera_type, const float* cam, const float* sR, const float* t, float x, float y, float z, float uv[2]) {
#pragma clang fp contract(off)
  const float v[3] = {((sR[0] * x + sR[1] * y) + sR[2] * z) + t[0], ((sR[3] * x + sR[4] * y) + sR[5] * z) + t[1],
                      ((sR[6] * x + sR[7] * y) + sR[8] * z) + t[2]};
  const Pixel p = ransac_project(camera_type, cam, v);
  uv[0] = p.u; uv[1] = p.v;
}
// X1, X2: the point in camera 1 and camera 2; p1, p2: its pixels in image 1 and image 2
OSH_KB8_HD bool s3r_inlier(int type1, const float* cam1, int type2, const float* cam2, const S3rTransform& T, const float* X1, const float* X2,
                           const float* p1, const float* p2, float max1, float max2) {
#pragma clang fp contract(off)
  float p2im1[2], p1im2[2];
  s3r_project(type1, cam1, T.sR, T.t, X2[0], X2[1], X2[2], p2im1);
  s3r_project(type2, cam2, T.sRinv, T.tinv, X1[0], X1[1], X1[2], p1im2);
  const float d1x = p1[0] - p2im1[0], d1y = p1[1] - p2im1[1], d2x = p1im2[0] - p2[0], d2y = p1im2[1] - p2[1];
  const float err1 = d1x * d1x + d1y * d1y, err2 = d2x * d2x + d2y * d2y;
  return err1 < max1 && err2 < max2;
}

// ---------------------------------------------------------------------------------------------------- iterate (:167-210, :240-288)
// record[0..n_records): the iterations that are records; H: first_hit, n_records, the best at the end
OSH_KB8_HD void s3r_scan_records(const int* count, int n_iter, int min_inliers, int best_in, int* record, S3rHead& H) {
  int best = best_in, n_rec = 0, hit = -1, last = -1;
  for (int k = 0; k < n_iter; ++k)
    if (count[k] >= best) {
      best = count[k]; record[n_rec++] = k; last = k;
      if (hit < 0 && count[k] > min_inliers) hit = k;
    }
  H.first_hit = hit; H.n_records = n_rec; H.best_iteration = last; H.best_count = best;
}

// SetRansacParameters (:123-147): mRansacMaxIts for N correspondences.  epsilon is a float as in the reference (inf for N = 0),
// pow(epsilon, 3) the double power of the float
inline int s3r_max_iterations(int N, double probability, int minInliers, int maxIterations) {
  const float epsilon = (float)minInliers / (float)N;
  int nIterations = 1;
  if (minInliers != N) {
    const double v = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3)));
    nIterations = v == v && v > -2147483648.0 && v < 2147483647.0 ? (int)v : INT32_MIN;   // what the conversion gives on x86-64
  }
  return std::max(1, std::min(nIterations, maxIterations));
}

// ---------------------------------------------------------------------------------------------------- the host build
inline void s3r_gather_set(const osh_sim3r_problem& P, const int32_t* set, float* P1, float* P2) {
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) { P1[3 * k + i] = P.x3dc1[3 * (size_t)set[k] + i]; P2[3 * k + i] = P.x3dc2[3 * (size_t)set[k] + i]; }
}
// CheckInliers of one transform (13 floats) over the n correspondences: the count, the mask as bit words (bit i % 32 of word i / 32)
inline int s3r_check_inliers_host(const osh_sim3r_problem& P, const float* T13, uint32_t* mask) {
  const int words = ransac_mask_words(P.n);
  S3rTransform T;
  s3r_transforms(T13, T13 + 9, T13[12], T);
  int count = 0;
  for (int w = 0; w < words; ++w) mask[w] = 0;
  for (int i = 0; i < P.n; ++i) {
    const size_t j = (size_t)i;
    if (s3r_inlier(P.camera_type1, P.camera1, P.camera_type2, P.camera2, T, P.x3dc1 + 3 * j, P.x3dc2 + 3 * j, P.p1im1 + 2 * j, P.p2im2 + 2 * j,
                   P.max_error1[i], P.max_error2[i])) { mask[i >> 5] |= 1u << (i & 31); ++count; }
  }
  return count;
}

inline void s3r_write_head(const osh_sim3r_result& r, const S3rHead& H) {
  if (r.first_hit) *r.first_hit = H.first_hit;
  if (r.n_records) *r.n_records = H.n_records;
  if (r.best_iteration) *r.best_iteration = H.best_iteration;
  if (r.best_count) *r.best_count = H.best_count;
}

// osh_orb_sim3_ransac for one valid problem, on one thread
inline void s3r_solve_host(const osh_sim3r_problem& P, const osh_sim3r_result& r) {
  const int n_it = P.n_iterations, words = ransac_mask_words(P.n);
  const size_t ni = (size_t)n_it, nw = (size_t)words;
  std::vector<float> T(ni * 13 + 13), rec_T(ni * 13 + 13, 0.f);
  std::vector<int> count(ni + 1), record(ni + 1, -1), rec_count(ni + 1, 0);
  std::vector<uint32_t> mask(ni * nw + 2), rec_mask(ni * nw + 2, 0u);
  for (int k = 0; k < n_it; ++k) {
    float P1[9], P2[9];
    s3r_gather_set(P, P.sets + 3 * (size_t)k, P1, P2);
    s3r_compute_sim3(P1, P2, P.fix_scale != 0, &T[13 * (size_t)k]);
    count[k] = s3r_check_inliers_host(P, &T[13 * (size_t)k], &mask[(size_t)k * nw]);
  }
  S3rHead H;
  s3r_scan_records(count.data(), n_it, P.min_inliers, P.best_inliers_in, record.data(), H);
  for (int q = 0; q < H.n_records; ++q) {
    const size_t k = (size_t)record[q];
    rec_count[q] = count[k];
    std::memcpy(&rec_T[13 * (size_t)q], &T[13 * k], 13 * sizeof(float));
    if (nw) std::memcpy(&rec_mask[(size_t)q * nw], &mask[k * nw], nw * sizeof(uint32_t));
  }
  for (size_t q = (size_t)H.n_records; q < ni; ++q) record[q] = -1;
  s3r_write_head(r, H);
  copy_if(r.record, record.data(), ni);
  copy_if(r.record_count, rec_count.data(), ni);
  copy_if(r.record_T, rec_T.data(), ni * 13);
  copy_if(r.record_mask, rec_mask.data(), ni * nw);
  copy_if(r.debug_count, count.data(), ni);
  copy_if(r.debug_T, T.data(), ni * 13);
}

}  // namespace osh
