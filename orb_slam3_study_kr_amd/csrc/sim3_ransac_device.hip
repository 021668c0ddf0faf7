// sim3_ransac_device.hip -- Sim3Solver::iterate (src/Sim3Solver.cc:149-294), the Sim3 RANSAC of loop closing and map merging, on
// MI355X (gfx950) for a batch of problems; the statements are those of sim3_ransac.h.  One upload, two launches with no host decision
// between them, one download:
//   k_s3r_hypothesis  one wavefront per (iteration, problem).  Every lane forms the hypothesis of the minimal set (ComputeSim3: uniform
//                     work, no LDS, no cross-lane step), then lane l scores the correspondences l, l + 64, ..: both projections and
//                     both tests, the mask words from the ballot, the count from its population count.  The correspondences of the
//                     batch are twelve float arrays (structure of arrays), so a wavefront's loads are contiguous.  Also runs alone,
//                     on given transforms, behind osh_orb_sim3_ransac_check_inliers.
//   k_s3r_decide      one wavefront per problem: the running best as a prefix maximum over the counts, the records from a ballot,
//                     first_hit, the best at the end; every record's count, transform and mask words compacted to its ordinal, the
//                     unused record slots cleared.
// Every output word is written by these kernels, so nothing has to be preset.
#include "common.h"
#include "sim3_ransac.h"
#include "orb_stage.h"
#include <climits>
#include <vector>

namespace osh {

enum { kS3rX1 = 0, kS3rX2 = 3, kS3rP1 = 6, kS3rP2 = 8, kS3rE1 = 10, kS3rE2 = 11, kS3rArrays = 12 };

struct S3rView {
  const S3rProblem* prob;
  const float* soa;   // array c of the batch at soa + c * total: x1 y1 z1 x2 y2 z2 u1 v1 u2 v2 max1 max2
  int total;          // correspondences of the batch
  const int* sets;    // [iterations of the batch][3]
  float* T; int* count; unsigned* mask;   // per (problem, iteration): base_h + it; mask words at base_w + it * words
  int* record; int* rec_count; float* rec_T; unsigned* rec_mask;   // per (problem, record): the same offsets
  S3rHead* head;
};

// grid = (max iterations, n_problems).  given: the transforms to score (the hypotheses are not formed), or null
__global__ __launch_bounds__(kS3rWave) void k_s3r_hypothesis(S3rView v, const float* given) {
  const S3rProblem& P = v.prob[blockIdx.y];
  const int it = blockIdx.x, lane = threadIdx.x, n = P.n;
  if (it >= P.n_iter) return;
  const size_t g = (size_t)P.base_h + it, total = (size_t)v.total;
  const float* soa = v.soa + P.base_p;
  float T13[13];
  if (given) {
#pragma unroll
    for (int k = 0; k < 13; ++k) T13[k] = given[13 * g + k];
  } else {
    float P1[9], P2[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int idx = v.sets[3 * g + k];
#pragma unroll
      for (int i = 0; i < 3; ++i) { P1[3 * k + i] = soa[(kS3rX1 + i) * total + idx]; P2[3 * k + i] = soa[(kS3rX2 + i) * total + idx]; }
    }
    s3r_compute_sim3(P1, P2, P.fix_scale != 0, T13);
  }
  S3rTransform T;
  s3r_transforms(T13, T13 + 9, T13[12], T);
  float cam1[8], cam2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { cam1[k] = P.cam1[k]; cam2[k] = P.cam2[k]; }
  const int c = wave_score(lane, n, v.mask + (size_t)P.base_w + (size_t)it * P.words, [&](int i) {
    const float X1[3] = {soa[(kS3rX1 + 0) * total + i], soa[(kS3rX1 + 1) * total + i], soa[(kS3rX1 + 2) * total + i]};
    const float X2[3] = {soa[(kS3rX2 + 0) * total + i], soa[(kS3rX2 + 1) * total + i], soa[(kS3rX2 + 2) * total + i]};
    const float p1[2] = {soa[(kS3rP1 + 0) * total + i], soa[(kS3rP1 + 1) * total + i]};
    const float p2[2] = {soa[(kS3rP2 + 0) * total + i], soa[(kS3rP2 + 1) * total + i]};
    return s3r_inlier(P.camera_type1, cam1, P.camera_type2, cam2, T, X1, X2, p1, p2, soa[kS3rE1 * total + i], soa[kS3rE2 * total + i]);
  });
  if (lane == 0) {
    v.count[g] = c;
    if (!given) {
#pragma unroll
      for (int k = 0; k < 13; ++k) v.T[13 * g + k] = T13[k];
    }
  }
}

// grid = n_problems
__global__ __launch_bounds__(kS3rWave) void k_s3r_decide(S3rView v) {
  const S3rProblem& P = v.prob[blockIdx.x];
  const int lane = threadIdx.x, n_it = P.n_iter, words = P.words;
  const size_t bh = (size_t)P.base_h, bw = (size_t)P.base_w;
  __shared__ int s_rec[OSH_SIM3R_MAX_ITERATIONS];
  int best = P.best_in, hit = -1, last = -1;
  const int n_rec = wave_compact(lane, n_it, [&](int k) {   // 64 iterations at a time: is k a record?
    const int base = k - lane;
    const int c = k < n_it ? v.count[bh + k] : INT_MIN;
    int m = c;   // the maximum over the lanes up to this one
#pragma unroll
    for (int d = 1; d < kS3rWave; d *= 2) {
      const int o = __shfl_up(m, d);
      if (lane >= d) m = max(m, o);
    }
    const int before = __shfl_up(m, 1);
    const int running = lane == 0 ? best : max(best, before);   // s3r_scan_records' `best` when it reaches k
    const bool rec = k < n_it && c >= running;
    const unsigned long long b = __ballot(rec), h = __ballot(rec && c > P.min_inliers);
    if (hit < 0 && h) hit = base + __ffsll((long long)h) - 1;
    if (b) last = base + 63 - __clzll((long long)b);
    best = max(best, __shfl(m, kS3rWave - 1));
    return rec;
  }, s_rec);
  __syncthreads();
  if (lane == 0) {
    S3rHead& H = v.head[blockIdx.x];
    H.first_hit = hit; H.n_records = n_rec; H.best_iteration = last; H.best_count = best;
  }
  for (int q = lane; q < n_it; q += kS3rWave) {
    const size_t g = bh + q;
    const int k = q < n_rec ? s_rec[q] : -1;
    v.record[g] = k;
    v.rec_count[g] = k >= 0 ? v.count[bh + k] : 0;
    for (int j = 0; j < 13; ++j) v.rec_T[13 * g + j] = k >= 0 ? v.T[13 * (bh + k) + j] : 0.f;
  }
  if (words > 0) {
    for (int e = lane; e < n_it * words; e += kS3rWave) {
      const int q = e / words, w = e - q * words;
      v.rec_mask[bw + e] = q < n_rec ? v.mask[bw + (size_t)s_rec[q] * words + w] : 0u;
    }
  }
}

struct Sim3RansacState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
};

static int s3r_validate_points(const char* entry, int k, const osh_sim3r_problem& p) {
  if (p.n < 0) { set_error("%s: problem %d: negative count", entry, k); return OSH_ERR_INVALID; }
  if (p.n > OSH_SIM3R_MAX_POINTS) { set_error("%s: problem %d: more than %d correspondences", entry, k, OSH_SIM3R_MAX_POINTS); return OSH_ERR_UNSUPPORTED; }
  for (int t : {p.camera_type1, p.camera_type2})
    if (t != OSH_SIM3R_PINHOLE && t != OSH_SIM3R_KB8) { set_error("%s: problem %d: camera type %d", entry, k, t); return OSH_ERR_INVALID; }
  if (p.n && (!p.x3dc1 || !p.x3dc2 || !p.p1im1 || !p.p2im2 || !p.max_error1 || !p.max_error2)) {
    set_error("%s: problem %d: NULL array with n = %d", entry, k, p.n);
    return OSH_ERR_INVALID;
  }
  return OSH_OK;
}

static int s3r_validate(int n_problems, const osh_sim3r_problem* ps, RansacBatch& batch) {
  const char* entry = "osh_orb_sim3_ransac";
  if (n_problems > OSH_SIM3R_MAX_PROBLEMS) { set_error("%s: more than %d problems", entry, OSH_SIM3R_MAX_PROBLEMS); return OSH_ERR_UNSUPPORTED; }
  batch.base.reserve((size_t)n_problems);
  for (int k = 0; k < n_problems; ++k) {
    const osh_sim3r_problem& p = ps[k];
    OSH_TRY(s3r_validate_points(entry, k, p));
    if (p.n_iterations < 0) { set_error("%s: problem %d: negative count", entry, k); return OSH_ERR_INVALID; }
    if (p.n_iterations > OSH_SIM3R_MAX_ITERATIONS) { set_error("%s: problem %d: more than %d iterations", entry, k, OSH_SIM3R_MAX_ITERATIONS); return OSH_ERR_UNSUPPORTED; }
    OSH_TRY(validate_minimal_sets<3>(entry, k, p.sets, p.n_iterations, p.n));
    batch.add(p.n, p.n_iterations, ransac_mask_words(p.n));
  }
  return OSH_OK;
}

static void s3r_fill_problem(S3rProblem& d, const osh_sim3r_problem& p, int n_iter, size_t base_p, size_t base_h, size_t base_w) {
  d.camera_type1 = p.camera_type1; d.camera_type2 = p.camera_type2;
  for (int k = 0; k < 8; ++k) { d.cam1[k] = p.camera1[k]; d.cam2[k] = p.camera2[k]; }
  d.fix_scale = p.fix_scale ? 1 : 0;
  d.n = p.n; d.n_iter = n_iter; d.min_inliers = p.min_inliers; d.best_in = p.best_inliers_in;
  d.words = ransac_mask_words(p.n);
  d.base_p = (int)base_p; d.base_h = (int)base_h; d.base_w = (int)base_w;
}

// The correspondences of one problem into the twelve arrays of the batch (each `total` long), from correspondence base_p on
static void s3r_stage_points(float* soa, size_t total, size_t base_p, const osh_sim3r_problem& p) {
  float* a = soa + base_p;
  for (size_t i = 0; i < (size_t)p.n; ++i) {
    for (int c = 0; c < 3; ++c) { a[(kS3rX1 + c) * total + i] = p.x3dc1[3 * i + c]; a[(kS3rX2 + c) * total + i] = p.x3dc2[3 * i + c]; }
    for (int c = 0; c < 2; ++c) { a[(kS3rP1 + c) * total + i] = p.p1im1[2 * i + c]; a[(kS3rP2 + c) * total + i] = p.p2im2[2 * i + c]; }
    a[kS3rE1 * total + i] = p.max_error1[i]; a[kS3rE2 * total + i] = p.max_error2[i];
  }
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_sim3_ransac(osh_orb_ctx* c, int32_t n_problems, const osh_sim3r_problem* ps, const osh_sim3r_result* results) {
  PhaseClock clock;
  if (n_problems < 0 || (n_problems && (!ps || !results))) { set_error("osh_orb_sim3_ransac: bad arguments"); return OSH_ERR_INVALID; }
  RansacBatch batch;
  OSH_TRY(s3r_validate(n_problems, ps, batch));   // the problems first: a refusal needs no context and no device
  if (!c) { set_error("osh_orb_sim3_ransac: no context"); return OSH_ERR_INVALID; }
  if (n_problems == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  Sim3RansacState* st = orb_state<Sim3RansacState>(c, kOrbAttachSim3Ransac);
  clock.profiling = orb_profiling(c);
  bool debug = false;
  for (int k = 0; k < n_problems; ++k) debug = debug || results[k].debug_T;

  const size_t nP = (size_t)n_problems, N = batch.N, I = batch.I, W = batch.W;
  Layout in, out, work;
  const auto s_prob = in.take<S3rProblem>(nP);
  const auto s_soa = in.take<float>(N * kS3rArrays);
  const auto s_sets = in.take<int>(I * 3);
  const auto o_head = out.take<S3rHead>(nP);
  const auto o_count = out.take<int>(I); const auto o_record = out.take<int>(I); const auto o_rcount = out.take<int>(I);
  const auto o_rT = out.take<float>(I * 13);
  const auto o_rmask = out.take<unsigned>(W);
  // the transforms of all iterations are results only when a caller asks for debug_T; otherwise they stay on the device
  const auto h_T = (debug ? out : work).take<float>(I * 13);
  const auto w_mask = work.take<unsigned>(W);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  for (int k = 0; k < n_problems; ++k) {
    const RansacBatch::Base& b = batch.base[k];
    s3r_fill_problem(s_prob.in(h)[k], ps[k], ps[k].n_iterations, b.p, b.h, b.w);
    s3r_stage_points(s_soa.in(h), N, b.p, ps[k]);
  }
  batch.stage_sets<3>(s_sets.in(h), ps);
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  char* dw = st->call.dev_work();
  S3rView v{};
  v.prob = s_prob.in(di); v.soa = s_soa.in(di); v.total = (int)N; v.sets = s_sets.in(di);
  v.T = h_T.in(debug ? dout : dw); v.count = o_count.in(dout); v.mask = w_mask.in(dw);
  v.record = o_record.in(dout); v.rec_count = o_rcount.in(dout); v.rec_T = o_rT.in(dout); v.rec_mask = o_rmask.in(dout);
  v.head = o_head.in(dout);
  const dim3 per_iteration((unsigned)std::max(batch.max_iter, 1), (unsigned)n_problems), per_problem((unsigned)n_problems), wave(kS3rWave);
  hipLaunchKernelGGL(k_s3r_hypothesis, per_iteration, wave, 0, s, v, (const float*)nullptr);
  OSH_TRY(launch_check("Sim3 RANSAC hypotheses"));
  hipLaunchKernelGGL(k_s3r_decide, per_problem, wave, 0, s, v);
  OSH_TRY(launch_check("Sim3 RANSAC decision"));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_problems; ++k) {
    const osh_sim3r_result& r = results[k];
    const size_t ni = (size_t)ps[k].n_iterations, words = (size_t)ransac_mask_words(ps[k].n), bh = batch.base[k].h;
    s3r_write_head(r, o_head.in(ho)[k]);
    scatter(r.record, o_record, ho, bh, ni); scatter(r.record_count, o_rcount, ho, bh, ni);
    scatter(r.record_T, o_rT, ho, bh, ni, 13);
    scatter(r.record_mask, o_rmask, ho, batch.base[k].w, ni * words);
    scatter(r.debug_count, o_count, ho, bh, ni);
    if (debug) scatter(r.debug_T, h_T, ho, bh, ni, 13);
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_sim3_ransac_check_inliers(osh_orb_ctx* c, const osh_sim3r_problem* p, int32_t n_T, const float* T12s, int32_t* count,
                                                 uint32_t* mask) {
  const char* entry = "osh_orb_sim3_ransac_check_inliers";
  if (!p || n_T < 0 || (n_T && (!T12s || !count || !mask))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  OSH_TRY(s3r_validate_points(entry, 0, *p));
  if (n_T > OSH_SIM3R_MAX_ITERATIONS) { set_error("%s: more than %d transforms", entry, OSH_SIM3R_MAX_ITERATIONS); return OSH_ERR_UNSUPPORTED; }
  if (!c) { set_error("%s: no context", entry); return OSH_ERR_INVALID; }
  if (n_T == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  Sim3RansacState* st = orb_state<Sim3RansacState>(c, kOrbAttachSim3Ransac);
  const size_t n = (size_t)p->n, nt = (size_t)n_T, words = (size_t)ransac_mask_words(p->n);
  Layout in, out;
  const auto s_prob = in.take<S3rProblem>(1);
  const auto s_soa = in.take<float>(n * kS3rArrays);
  const auto s_T = in.take<float>(nt * 13);
  const auto o_count = out.take<int>(nt); const auto o_mask = out.take<unsigned>(nt * words);
  OSH_TRY(st->call.reserve(in, out, 0));
  char* h = st->call.host_in();
  s3r_fill_problem(*s_prob.in(h), *p, n_T, 0, 0, 0);
  s3r_stage_points(s_soa.in(h), n, 0, *p);
  std::memcpy(s_T.in(h), T12s, nt * 13 * sizeof(float));
  OSH_TRY(st->call.upload(s));
  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  S3rView v{};
  v.prob = s_prob.in(di); v.soa = s_soa.in(di); v.total = (int)n;
  v.count = o_count.in(dout); v.mask = o_mask.in(dout);
  hipLaunchKernelGGL(k_s3r_hypothesis, dim3((unsigned)n_T, 1), dim3(kS3rWave), 0, s, v, (const float*)s_T.in(di));
  OSH_TRY(launch_check("Sim3 RANSAC scoring"));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  std::memcpy(count, o_count.in(ho), nt * 4);
  if (words) std::memcpy(mask, o_mask.in(ho), nt * words * 4);
  return OSH_OK;
}

extern "C" int osh_orb_sim3_ransac_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<Sim3RansacState>("osh_orb_sim3_ransac_get_times", c, kOrbAttachSim3Ransac, ms);
}
