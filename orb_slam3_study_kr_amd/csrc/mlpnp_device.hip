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
__device__ __forceinline__ double ml_rows_sum(double x) {   // tv_tree16 over lanes 0..15, the result in every lane
#pragma clang fp contract(off)
  x = x + __shfl_xor(x, 1);
  x = x + __shfl_xor(x, 2);
  x = x + __shfl_xor(x, 4);
  x = x + __shfl_xor(x, 8);
  return __shfl(x, 0);
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
  for (int sweep = 0; sweep < kMlSweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < 11; ++p)
#pragma unroll
      for (int q = p + 1; q < 12; ++q) {
        const double alpha = ml_rows_sum(row[p] * row[p]), beta = ml_rows_sum(row[q] * row[q]), gamma = ml_rows_sum(row[p] * row[q]);
        double c, s;
        tv_rotation(alpha, beta, gamma, c, s);
        tv_rotate_pair(row[p], row[q], c, s);
      }
  }
  const int cols = planar ? 9 : 12;
  int best = 0;
  double best_n = 0;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const double nj = ml_rows_sum(row[j] * row[j]);
    if (j < cols && (j == 0 || nj < best_n)) { best_n = nj; best = j; }
  }
  double mine = 0;
#pragma unroll
  for (int j = 0; j < 12; ++j) if (j == best) mine = row[j];
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
  unsigned* m = mask + (size_t)P.base_w + (size_t)it * P.words;
  int c = 0;
  for (int base = 0; base < n; base += kMlWave) {
    const int i = base + lane;
    bool in = false;
    if (i < n) {
      const size_t j = (size_t)P.base_p + i;
      in = ml_inlier(P.camera_type, cam, T, v.p3d + 3 * j, v.p2d + 2 * j, v.max_error[j]);
    }
    const unsigned long long b = __ballot(in);
    if (lane == 0) { m[base >> 5] = (unsigned)b; m[(base >> 5) + 1] = (unsigned)(b >> 32); }
    c += __popcll(b);
  }
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
  int c = 0;
  for (int base = 0; base < n; base += kMlWave) {
    const int i = base + lane;
    const bool in = i < n && ((m[i >> 5] >> (i & 31)) & 1u);
    const unsigned long long b = __ballot(in);
    if (in) s_idx[c + __popcll(b & ((1ull << lane) - 1ull))] = i;
    c += __popcll(b);
  }
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

static int ml_validate(int n_problems, const osh_mlpnp_problem* ps, size_t* total_n, size_t* total_i, size_t* total_w, size_t* total_o, int* max_iter) {
  const char* entry = "osh_orb_mlpnp_solve";
  if (n_problems > OSH_MLPNP_MAX_PROBLEMS) { set_error("%s: more than %d problems", entry, OSH_MLPNP_MAX_PROBLEMS); return OSH_ERR_UNSUPPORTED; }
  size_t N = 0, I = 0, W = 0, O = 0;
  int mx = 0;
  for (int k = 0; k < n_problems; ++k) {
    const osh_mlpnp_problem& p = ps[k];
    OSH_TRY(ml_validate_points(entry, k, p));
    if (p.n_iterations < 0) { set_error("%s: problem %d: negative count", entry, k); return OSH_ERR_INVALID; }
    if (p.n_iterations > OSH_MLPNP_MAX_ITERATIONS) { set_error("%s: problem %d: more than %d iterations", entry, k, OSH_MLPNP_MAX_ITERATIONS); return OSH_ERR_UNSUPPORTED; }
    if (p.min_inliers < 6) { set_error("%s: problem %d: min_inliers %d below the minimal set of 6", entry, k, p.min_inliers); return OSH_ERR_INVALID; }
    if (p.n_iterations && !p.sets) { set_error("%s: problem %d: NULL sets with n_iterations = %d", entry, k, p.n_iterations); return OSH_ERR_INVALID; }
    if (p.n_iterations && p.n < 6) { set_error("%s: problem %d: %d correspondences cannot fill a minimal set of 6", entry, k, p.n); return OSH_ERR_INVALID; }
    for (int it = 0; it < p.n_iterations; ++it) {
      const int32_t* s = p.sets + 6 * (size_t)it;
      for (int a = 0; a < 6; ++a) {
        if (s[a] < 0 || s[a] >= p.n) { set_error("%s: problem %d: set %d: index %d outside [0, %d)", entry, k, it, s[a], p.n); return OSH_ERR_INVALID; }
        for (int b = 0; b < a; ++b)
          if (s[a] == s[b]) { set_error("%s: problem %d: set %d repeats index %d", entry, k, it, s[a]); return OSH_ERR_INVALID; }
      }
    }
    const size_t words = (size_t)OSH_MLPNP_MASK_WORDS(p.n);
    N += (size_t)p.n; I += (size_t)p.n_iterations; W += words * (size_t)p.n_iterations; O += words;
    mx = std::max(mx, p.n_iterations);
  }
  *total_n = N; *total_i = I; *total_w = W; *total_o = O; *max_iter = mx;
  return OSH_OK;
}

static void ml_fill_problem(MlProblem& d, const osh_mlpnp_problem& p, int n_iter, size_t base_p, size_t base_h, size_t base_w) {
  d.camera_type = p.camera_type;
  for (int k = 0; k < 8; ++k) d.cam[k] = p.camera[k];
  d.n = p.n; d.n_iter = n_iter; d.min_inliers = p.min_inliers; d.best_in = p.best_inliers_in; d.ok_in = p.best_refine_ok_in ? 1 : 0;
  d.words = OSH_MLPNP_MASK_WORDS(p.n);
  d.base_p = (int)base_p; d.base_h = (int)base_h; d.base_w = (int)base_w;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_mlpnp_solve(osh_orb_ctx* c, int32_t n_problems, const osh_mlpnp_problem* ps, const osh_mlpnp_result* results) {
  PhaseClock clock;
  if (n_problems < 0 || (n_problems && (!ps || !results))) { set_error("osh_orb_mlpnp_solve: bad arguments"); return OSH_ERR_INVALID; }
  size_t N = 0, I = 0, W = 0, O = 0;
  int max_iter = 0;
  OSH_TRY(ml_validate(n_problems, ps, &N, &I, &W, &O, &max_iter));   // the problems first: a refusal needs no context and no device
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

  const size_t nP = (size_t)n_problems;
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
  std::vector<size_t> base_p(nP), base_h(nP), base_o(nP);
  size_t bp = 0, bh = 0, bw = 0, bo = 0;
  for (int k = 0; k < n_problems; ++k) {
    const osh_mlpnp_problem& p = ps[k];
    const size_t n = (size_t)p.n, ni = (size_t)p.n_iterations, words = (size_t)OSH_MLPNP_MASK_WORDS(p.n);
    base_p[k] = bp; base_h[k] = bh; base_o[k] = bo;
    ml_fill_problem(s_prob.in(h)[k], p, p.n_iterations, bp, bh, bw);
    s_base_o.in(h)[k] = (int)bo;
    if (n) {
      std::memcpy(s_bearing.in(h) + bp * 3, p.bearing, n * 24); std::memcpy(s_p3d.in(h) + bp * 3, p.p3d, n * 24);
      std::memcpy(s_p2d.in(h) + bp * 2, p.p2d, n * 8); std::memcpy(s_err.in(h) + bp, p.max_error, n * 4);
    }
    if (ni) std::memcpy(s_sets.in(h) + bh * 6, p.sets, ni * 24);
    bp += n; bh += ni; bw += words * ni; bo += words;
  }
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
  const dim3 per_pose((unsigned)std::max(max_iter, 1), (unsigned)n_problems), per_problem((unsigned)n_problems), wave(kMlWave);
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
    const size_t ni = (size_t)ps[k].n_iterations, words = (size_t)OSH_MLPNP_MASK_WORDS(ps[k].n);
    ml_write_head(r, o_head.in(ho)[k]);
    scatter(r.hit_mask, o_hit, ho, base_o[k], words); scatter(r.best_mask, o_best, ho, base_o[k], words);
    scatter(r.debug_count, o_count, ho, base_h[k], ni); scatter(r.debug_record, o_record, ho, base_h[k], ni);
    scatter(r.debug_record_count, o_rcount, ho, base_h[k], ni);
    if (debug) { scatter(r.debug_pose, h_pose, ho, base_h[k], ni, 12); scatter(r.debug_record_pose, h_rpose, ho, base_h[k], ni, 12); }
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
  const size_t n = (size_t)p->n, np = (size_t)n_poses, words = (size_t)OSH_MLPNP_MASK_WORDS(p->n);
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
  if (!c || !ms) { set_error("osh_orb_mlpnp_get_times: bad arguments"); return OSH_ERR_INVALID; }
  std::memcpy(ms, orb_state<MlpnpState>(c, kOrbAttachMlpnp)->ms, sizeof(double) * 5);
  return OSH_OK;
}
