// mlpnp_device.hip -- MLPnPsolver::iterate (src/MLPnPsolver.cpp:100-353), the PnP RANSAC of relocalisation, on MI355X (gfx950) for a
// batch of problems; the statements are those of mlpnp.h.  One upload, six launches with no host decision between them, one download:
//   k_ml_hypothesis  one wavefront per (iteration, problem): computePose of the minimal set.  Sums over the correspondences are one
//                    partial per lane joined by six xor-butterfly steps (the pairwise tree ml_tree64 states); the 12x12 normal matrix
//                    lives one row per lane in lanes 0..11 and V one row per lane in lanes 16..27, a column pair's three sums are four
//                    butterfly steps across 16 lanes and the 66 pairs of a sweep are unrolled, so the rows stay in registers; the
//                    3x3 factorisations, the candidate poses and the 6x6 solve are computed by every lane alike.
//   k_ml_score       one wavefront per (pose, problem): CheckInliers of 64 correspondences at a time, the mask words from the ballot,
//                    the count from its population count.  Runs on the hypotheses, later on the refined poses, and alone behind
//                    osh_orb_mlpnp_check_inliers.
//   k_ml_scan        one wavefront per problem: the records in iteration order; the unused record slots are cleared.
//   k_ml_refine      one wavefront per (record, problem): the record's inliers in ascending order into LDS (ballot prefix), then the
//                    same computePose over them.
//   k_ml_decide      one wavefront per problem: lane 0 takes the decision, all lanes copy the two masks out.
// Every output word is written by these kernels, so nothing has to be preset.
#include "common.h"
#include "mlpnp.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

struct MlView {
  const MlProblem* prob;
  const double* bearing; const double* p3d;   // [correspondences of the batch][3]
  const float* p2d; const float* max_error;   // [..][2], [..]
  const int* sets;                            // [iterations of the batch][6]
  double* pose; int* count; unsigned* mask;   // per (problem, iteration): base_h + it; mask words at base_w + it * words
  int* record; double* rec_pose; int* rec_count; unsigned* rec_mask;   // per (problem, record): the same offsets
  MlHead* head;
  unsigned* out_hit_mask; unsigned* out_best_mask;   // per problem: base_o
  const int* base_o;
};

__device__ __forceinline__ double ml_wave_sum(double x) {   // ml_tree64 over the 64 lanes, the result in every lane
#pragma clang fp contract(off)
  x = x + __shfl_xor(x, 1);
  x = x + __shfl_xor(x, 2);
  x = x + __shfl_xor(x, 4);
  x = x + __shfl_xor(x, 8);
  x = x + __shfl_xor(x, 16);
  x = x + __shfl_xor(x, 32);
  return x;
}

// computePose over the correspondences idx[0..n) (LDS) of the problem whose arrays start at bearing / p3d: what ml_compute_pose_host
// states, by one wavefront.  sT: 60 doubles of LDS.  The pose is left in every lane.
__device__ __forceinline__ void ml_compute_pose_wave(int lane, int n, const int* idx, const double* bearing, const double* p3d, double* sT,
                                                     double pose[12]) {
#pragma clang fp contract(off)
  double S[6] = {0, 0, 0, 0, 0, 0}, E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = lane; i < n; i += kMlWave) ml_add_planar(p3d + 3 * (size_t)idx[i], S);
#pragma unroll
  for (int k = 0; k < 6; ++k) S[k] = ml_wave_sum(S[k]);
  const bool planar = ml_rank3(S) == 2;
  if (planar) ml_eig3_rows(S, E);
  {
    double T[60];
#pragma unroll
    for (int k = 0; k < 60; ++k) T[k] = 0.0;
    for (int i = lane; i < n; i += kMlWave) ml_add_system(bearing + 3 * (size_t)idx[i], p3d + 3 * (size_t)idx[i], planar, E, T);
#pragma unroll
    for (int k = 0; k < 60; ++k) T[k] = ml_wave_sum(T[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 60; ++k) sT[k] = T[k];
    }
  }
  __syncthreads();
  double row[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) row[k] = lane < kMlRows ? (lane < 12 ? ml_system_entry(sT, planar, lane, k) : 0.0) : (lane - kMlRows == k ? 1.0 : 0.0);
  const double mine = null_vector_wave<12, kMlSweeps>(row, planar ? 9 : 12);
  double h[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) h[k] = __shfl(mine, kMlRows + k);

  double f6[18], p6[18], R[9], x[6];
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const size_t j = 3 * (size_t)idx[p];
#pragma unroll
    for (int k = 0; k < 3; ++k) { f6[3 * p + k] = bearing[j + k]; p6[3 * p + k] = p3d[j + k]; }
  }
  ml_initial_pose(planar, h, E, f6, p6, R, x + 3);
  ml_rot2rodrigues(R, x);
  for (int it = 0; it < kMlGnIterations; ++it) {
    MlGn g;
    ml_gn_setup(x, g);
    double H[27], dx[6];
#pragma unroll
    for (int k = 0; k < 27; ++k) H[k] = 0.0;
    for (int i = lane; i < n; i += kMlWave) ml_add_normal(g, bearing + 3 * (size_t)idx[i], p3d + 3 * (size_t)idx[i], H);
#pragma unroll
    for (int k = 0; k < 27; ++k) H[k] = ml_wave_sum(H[k]);
    ml_ldlt6(H, dx);
    if (ml_gn_spurious(dx)) break;   // dx is the same in every lane
    bool small = true;
    for (int i = lane; i < n; i += kMlWave) small = ml_update_small(g, bearing + 3 * (size_t)idx[i], p3d + 3 * (size_t)idx[i], dx) && small;
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = x[k] - dx[k];
    if (__all(small)) break;
  }
  double Jl[9];
  ml_rodrigues2rot(x, pose, Jl);
  pose[9] = x[3]; pose[10] = x[4]; pose[11] = x[5];
}

// grid = (max iterations, n_problems)
__global__ __launch_bounds__(kMlWave) void k_ml_hypothesis(MlView v) {
  const MlProblem& P = v.prob[blockIdx.y];
  const int it = blockIdx.x, lane = threadIdx.x;
  if (it >= P.n_iter) return;
  __shared__ int s_idx[8];
  __shared__ double s_T[60];
  const size_t g = (size_t)P.base_h + it;
  if (lane < 6) s_idx[lane] = v.sets[6 * g + lane];
  __syncthreads();
  double pose[12];
  ml_compute_pose_wave(lane, 6, s_idx, v.bearing + 3 * (size_t)P.base_p, v.p3d + 3 * (size_t)P.base_p, s_T, pose);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) v.pose[12 * g + k] = pose[k];
  }
}

// grid = (max poses, n_problems).  records: the poses are the refined ones of the problem's records
__global__ __launch_bounds__(kMlWave) void k_ml_score(MlView v, const double* poses, int* count, unsigned* mask, int records) {
  const MlProblem& P = v.prob[blockIdx.y];
  const int it = blockIdx.x, lane = threadIdx.x, n = P.n;
  if (it >= (records ? v.head[blockIdx.y].n_records : P.n_iter)) return;
  const size_t g = (size_t)P.base_h + it;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = poses[12 * g + k];
  float cam[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) cam[k] = P.cam[k];
  const int c = wave_score(lane, n, mask + (size_t)P.base_w + (size_t)it * P.words, [&](int i) {
    const size_t j = (size_t)P.base_p + i;
    return ml_inlier(P.camera_type, cam, T, v.p3d + 3 * j, v.p2d + 2 * j, v.max_error[j]);
  });
  if (lane == 0) count[g] = c;
}

// grid = n_problems
__global__ __launch_bounds__(kMlWave) void k_ml_scan(MlView v) {
  const MlProblem& P = v.prob[blockIdx.x];
  const int lane = threadIdx.x;
  __shared__ int s_rec;
  if (lane == 0) {
    s_rec = ml_scan_records(v.count + P.base_h, P.n_iter, P.min_inliers, P.best_in, v.record + P.base_h);
    v.head[blockIdx.x].n_records = s_rec;
  }
  __syncthreads();
  for (int q = s_rec + lane; q < P.n_iter; q += kMlWave) {
    const size_t g = (size_t)P.base_h + q;
    v.record[g] = -1; v.rec_count[g] = 0;
    for (int k = 0; k < 12; ++k) v.rec_pose[12 * g + k] = 0.0;
  }
}

// grid = (max iterations, n_problems)
__global__ __launch_bounds__(kMlWave) void k_ml_refine(MlView v) {
  const MlProblem& P = v.prob[blockIdx.y];
  const int q = blockIdx.x, lane = threadIdx.x, n = P.n;
  if (q >= v.head[blockIdx.y].n_records) return;
  __shared__ int s_idx[OSH_MLPNP_MAX_POINTS];
  __shared__ double s_T[60];
  const size_t g = (size_t)P.base_h + q;
  const unsigned* m = v.mask + (size_t)P.base_w + (size_t)v.record[g] * P.words;
  const int c = wave_compact(lane, n, [&](int i) { return i < n && ((m[i >> 5] >> (i & 31)) & 1u); }, s_idx);
  __syncthreads();
  double pose[12];
  ml_compute_pose_wave(lane, c, s_idx, v.bearing + 3 * (size_t)P.base_p, v.p3d + 3 * (size_t)P.base_p, s_T, pose);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) v.rec_pose[12 * g + k] = pose[k];
  }
}

// grid = n_problems
__global__ __launch_bounds__(kMlWave) void k_ml_decide(MlView v) {
  const MlProblem& P = v.prob[blockIdx.x];
  MlHead& H = v.head[blockIdx.x];
  const int lane = threadIdx.x;
  __shared__ int s_hit, s_best;
  if (lane == 0) {
    ml_decide(v.count + P.base_h, P.n_iter, P.min_inliers, P.best_in, P.ok_in, v.record + P.base_h, v.rec_count + P.base_h, H);
    H.pad = 0;
    for (int k = 0; k < 12; ++k) {
      H.hit_pose[k] = H.hit_record >= 0 ? v.rec_pose[12 * ((size_t)P.base_h + H.hit_record) + k] : 0.0;
      H.best_pose[k] = H.best_iteration >= 0 ? v.pose[12 * ((size_t)P.base_h + H.best_iteration) + k] : 0.0;
    }
    s_hit = H.hit_record; s_best = H.best_iteration;
  }
  __syncthreads();
  const int hit = s_hit, best = s_best;
  const size_t o = (size_t)v.base_o[blockIdx.x];
  for (int w = lane; w < P.words; w += kMlWave) {
    v.out_hit_mask[o + w] = hit >= 0 ? v.rec_mask[(size_t)P.base_w + (size_t)hit * P.words + w] : 0u;
    v.out_best_mask[o + w] = best >= 0 ? v.mask[(size_t)P.base_w + (size_t)best * P.words + w] : 0u;
  }
}

struct MlpnpState {
  StagedCall call;
  double ms[5] = {0, 0, 0, 0, 0};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~MlpnpState() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

static int ml_validate_points(const char* entry, int k, const osh_mlpnp_problem& p) {
  if (p.n < 0) { set_error("%s: problem %d: negative count", entry, k); return OSH_ERR_INVALID; }
  if (p.n > OSH_MLPNP_MAX_POINTS) { set_error("%s: problem %d: more than %d correspondences", entry, k, OSH_MLPNP_MAX_POINTS); return OSH_ERR_UNSUPPORTED; }
  if (p.camera_type != OSH_MLPNP_PINHOLE && p.camera_type != OSH_MLPNP_KB8) { set_error("%s: problem %d: camera type %d", entry, k, p.camera_type); return OSH_ERR_INVALID; }
  if (p.n && (!p.bearing || !p.p3d || !p.p2d || !p.max_error)) { set_error("%s: problem %d: NULL array with n = %d", entry, k, p.n); return OSH_ERR_INVALID; }
  return OSH_OK;
}

static int ml_validate(int n_problems, const osh_mlpnp_problem* ps, RansacBatch& batch) {
  const char* entry = "osh_orb_mlpnp_solve";
  if (n_problems > OSH_MLPNP_MAX_PROBLEMS) { set_error("%s: more than %d problems", entry, OSH_MLPNP_MAX_PROBLEMS); return OSH_ERR_UNSUPPORTED; }
  batch.base.reserve((size_t)n_problems);
  for (int k = 0; k < n_problems; ++k) {
    const osh_mlpnp_problem& p = ps[k];
    OSH_TRY(ml_validate_points(entry, k, p));
    if (p.n_iterations < 0) { set_error("%s: problem %d: negative count", entry, k); return OSH_ERR_INVALID; }
    if (p.n_iterations > OSH_MLPNP_MAX_ITERATIONS) { set_error("%s: problem %d: more than %d iterations", entry, k, OSH_MLPNP_MAX_ITERATIONS); return OSH_ERR_UNSUPPORTED; }
    if (p.min_inliers < 6) { set_error("%s: problem %d: min_inliers %d below the minimal set of 6", entry, k, p.min_inliers); return OSH_ERR_INVALID; }
    OSH_TRY(validate_minimal_sets<6>(entry, k, p.sets, p.n_iterations, p.n));
    batch.add(p.n, p.n_iterations, ransac_mask_words(p.n));
  }
  return OSH_OK;
}

static void ml_fill_problem(MlProblem& d, const osh_mlpnp_problem& p, int n_iter, size_t base_p, size_t base_h, size_t base_w) {
  d.camera_type = p.camera_type;
  for (int k = 0; k < 8; ++k) d.cam[k] = p.camera[k];
  d.n = p.n; d.n_iter = n_iter; d.min_inliers = p.min_inliers; d.best_in = p.best_inliers_in; d.ok_in = p.best_refine_ok_in ? 1 : 0;
  d.words = ransac_mask_words(p.n);
  d.base_p = (int)base_p; d.base_h = (int)base_h; d.base_w = (int)base_w;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_mlpnp_solve(osh_orb_ctx* c, int32_t n_problems, const osh_mlpnp_problem* ps, const osh_mlpnp_result* results) {
  PhaseClock clock;
  if (n_problems < 0 || (n_problems && (!ps || !results))) { set_error("osh_orb_mlpnp_solve: bad arguments"); return OSH_ERR_INVALID; }
  RansacBatch batch;
  OSH_TRY(ml_validate(n_problems, ps, batch));   // the problems first: a refusal needs no context and no device
  if (!c) { set_error("osh_orb_mlpnp_solve: no context"); return OSH_ERR_INVALID; }
  if (n_problems == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  MlpnpState* st = orb_state<MlpnpState>(c, kOrbAttachMlpnp);
  clock.profiling = orb_profiling(c);
  if (clock.profiling && !st->ev[0]) { OSH_HIP(hipEventCreate(&st->ev[0])); OSH_HIP(hipEventCreate(&st->ev[1])); }
  bool debug = false;
  for (int k = 0; k < n_problems; ++k) debug = debug || results[k].debug_pose || results[k].debug_record_pose;

  const size_t nP = (size_t)n_problems, N = batch.N, I = batch.I, W = batch.W;
  std::vector<size_t> base_o(nP);   // the two masks of a problem's result: one mask row per problem, beside the rows per iteration
  size_t O = 0;
  for (int k = 0; k < n_problems; ++k) { base_o[k] = O; O += (size_t)ransac_mask_words(ps[k].n); }
  Layout in, out, work;
  const auto s_prob = in.take<MlProblem>(nP);
  const auto s_base_o = in.take<int>(nP);
  const auto s_bearing = in.take<double>(N * 3); const auto s_p3d = in.take<double>(N * 3);
  const auto s_p2d = in.take<float>(N * 2); const auto s_err = in.take<float>(N);
  const auto s_sets = in.take<int>(I * 6);
  const auto o_head = out.take<MlHead>(nP);
  const auto o_hit = out.take<unsigned>(O); const auto o_best = out.take<unsigned>(O);
  const auto o_count = out.take<int>(I); const auto o_record = out.take<int>(I); const auto o_rcount = out.take<int>(I);
  // the poses are results only when a caller asks for the debug arrays; otherwise they stay on the device
  Layout& hyp = debug ? out : work;
  const auto h_pose = hyp.take<double>(I * 12); const auto h_rpose = hyp.take<double>(I * 12);
  const auto w_mask = work.take<unsigned>(W); const auto w_rmask = work.take<unsigned>(W);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  for (int k = 0; k < n_problems; ++k) {
    const osh_mlpnp_problem& p = ps[k];
    const size_t n = (size_t)p.n, bp = batch.base[k].p;
    ml_fill_problem(s_prob.in(h)[k], p, p.n_iterations, bp, batch.base[k].h, batch.base[k].w);
    s_base_o.in(h)[k] = (int)base_o[k];
    if (n) {
      std::memcpy(s_bearing.in(h) + bp * 3, p.bearing, n * 24); std::memcpy(s_p3d.in(h) + bp * 3, p.p3d, n * 24);
      std::memcpy(s_p2d.in(h) + bp * 2, p.p2d, n * 8); std::memcpy(s_err.in(h) + bp, p.max_error, n * 4);
    }
  }
  batch.stage_sets<6>(s_sets.in(h), ps);
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  char* dw = st->call.dev_work();
  char* dh = debug ? dout : dw;
  MlView v{};
  v.prob = s_prob.in(di); v.base_o = s_base_o.in(di);
  v.bearing = s_bearing.in(di); v.p3d = s_p3d.in(di); v.p2d = s_p2d.in(di); v.max_error = s_err.in(di); v.sets = s_sets.in(di);
  v.pose = h_pose.in(dh); v.rec_pose = h_rpose.in(dh);
  v.count = o_count.in(dout); v.record = o_record.in(dout); v.rec_count = o_rcount.in(dout);
  v.mask = w_mask.in(dw); v.rec_mask = w_rmask.in(dw);
  v.head = o_head.in(dout); v.out_hit_mask = o_hit.in(dout); v.out_best_mask = o_best.in(dout);
  const dim3 per_pose((unsigned)std::max(batch.max_iter, 1), (unsigned)n_problems), per_problem((unsigned)n_problems), wave(kMlWave);
  if (clock.profiling) OSH_HIP(hipEventRecord(st->ev[0], s));
  hipLaunchKernelGGL(k_ml_hypothesis, per_pose, wave, 0, s, v);
  OSH_TRY(launch_check("MLPnP hypotheses"));
  if (clock.profiling) OSH_HIP(hipEventRecord(st->ev[1], s));
  hipLaunchKernelGGL(k_ml_score, per_pose, wave, 0, s, v, (const double*)v.pose, v.count, v.mask, 0);
  OSH_TRY(launch_check("MLPnP scoring"));
  hipLaunchKernelGGL(k_ml_scan, per_problem, wave, 0, s, v);
  OSH_TRY(launch_check("MLPnP record scan"));
  hipLaunchKernelGGL(k_ml_refine, per_pose, wave, 0, s, v);
  OSH_TRY(launch_check("MLPnP refine"));
  hipLaunchKernelGGL(k_ml_score, per_pose, wave, 0, s, v, (const double*)v.rec_pose, v.rec_count, v.rec_mask, 1);
  OSH_TRY(launch_check("MLPnP refine scoring"));
  hipLaunchKernelGGL(k_ml_decide, per_problem, wave, 0, s, v);
  OSH_TRY(launch_check("MLPnP decision"));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_problems; ++k) {
    const osh_mlpnp_result& r = results[k];
    const size_t ni = (size_t)ps[k].n_iterations, words = (size_t)ransac_mask_words(ps[k].n), bh = batch.base[k].h;
    ml_write_head(r, o_head.in(ho)[k]);
    scatter(r.hit_mask, o_hit, ho, base_o[k], words); scatter(r.best_mask, o_best, ho, base_o[k], words);
    scatter(r.debug_count, o_count, ho, bh, ni); scatter(r.debug_record, o_record, ho, bh, ni);
    scatter(r.debug_record_count, o_rcount, ho, bh, ni);
    if (debug) { scatter(r.debug_pose, h_pose, ho, bh, ni, 12); scatter(r.debug_record_pose, h_rpose, ho, bh, ni, 12); }
  }
  clock.mark();
  clock.store(st->ms);
  if (clock.profiling) {
    float ms = 0.f;
    OSH_HIP(hipEventElapsedTime(&ms, st->ev[0], st->ev[1]));
    st->ms[4] = ms;
  }
  return OSH_OK;
}

extern "C" int osh_orb_mlpnp_check_inliers(osh_orb_ctx* c, const osh_mlpnp_problem* p, int32_t n_poses, const double* poses, int32_t* count,
                                           uint32_t* mask) {
  const char* entry = "osh_orb_mlpnp_check_inliers";
  if (!p || n_poses < 0 || (n_poses && (!poses || !count || !mask))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  OSH_TRY(ml_validate_points(entry, 0, *p));
  if (n_poses > OSH_MLPNP_MAX_ITERATIONS) { set_error("%s: more than %d poses", entry, OSH_MLPNP_MAX_ITERATIONS); return OSH_ERR_UNSUPPORTED; }
  if (!c) { set_error("%s: no context", entry); return OSH_ERR_INVALID; }
  if (n_poses == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  MlpnpState* st = orb_state<MlpnpState>(c, kOrbAttachMlpnp);
  const size_t n = (size_t)p->n, np = (size_t)n_poses, words = (size_t)ransac_mask_words(p->n);
  Layout in, out;
  const auto s_prob = in.take<MlProblem>(1);
  const auto s_p3d = in.take<double>(n * 3); const auto s_p2d = in.take<float>(n * 2); const auto s_err = in.take<float>(n);
  const auto s_pose = in.take<double>(np * 12);
  const auto o_count = out.take<int>(np); const auto o_mask = out.take<unsigned>(np * words);
  OSH_TRY(st->call.reserve(in, out, 0));
  char* h = st->call.host_in();
  ml_fill_problem(*s_prob.in(h), *p, n_poses, 0, 0, 0);
  if (n) { std::memcpy(s_p3d.in(h), p->p3d, n * 24); std::memcpy(s_p2d.in(h), p->p2d, n * 8); std::memcpy(s_err.in(h), p->max_error, n * 4); }
  std::memcpy(s_pose.in(h), poses, np * 96);
  OSH_TRY(st->call.upload(s));
  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  MlView v{};
  v.prob = s_prob.in(di); v.p3d = s_p3d.in(di); v.p2d = s_p2d.in(di); v.max_error = s_err.in(di);
  hipLaunchKernelGGL(k_ml_score, dim3((unsigned)n_poses, 1), dim3(kMlWave), 0, s, v, (const double*)s_pose.in(di), o_count.in(dout), o_mask.in(dout), 0);
  OSH_TRY(launch_check("MLPnP scoring"));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  std::memcpy(count, o_count.in(ho), np * 4);
  if (words) std::memcpy(mask, o_mask.in(ho), np * words * 4);
  return OSH_OK;
}

extern "C" int osh_orb_mlpnp_get_times(osh_orb_ctx* c, double ms[5]) {
  return copy_times<MlpnpState, 5>("osh_orb_mlpnp_get_times", c, kOrbAttachMlpnp, ms);
}
