// two_view_device.hip -- TwoViewReconstruction (src/TwoViewReconstruction.cc:41-927), the monocular initialisation, on MI355X (gfx950)
// for a batch of problems; the statements are those of two_view.h.  One upload, four launches with no host decision between them,
// one download:
//   k_tv_hypothesis  one wavefront per (iteration, model, problem).  The 16x9 system of the minimal set (8x9 and eight zero rows for
//                    F) lives one row per lane in lanes 0..15 and V one row per lane in lanes 16..24, so a column pair's three sums
//                    are four xor-butterfly steps across the 16 lanes (the pairwise tree tree16 states) and the rotation is two
//                    FP64 multiply-adds per lane (null_vector_wave of jacobi_rows.h: the 36 pairs of a sweep are unrolled so the rows
//                    stay in registers).  Then every
//                    lane forms the model, the lanes evaluate 64 matches at a time, and the terms are added in match order from LDS.
//   k_tv_select      one wavefront per problem: per model the first iteration with the strictly greatest score above 0, the branch,
//                    the inlier flags of the branch's model (recomputed from the stored model: the same statements, so the same
//                    flags as when it was scored), their count and the 8 or 4 motion hypotheses.
//   k_tv_check_rt    one block per (motion hypothesis, problem), the matches over its threads: CheckRT per inlier, nGood by an LDS
//                    counter, and the order statistic of the cosines by a four-pass radix select over their ordered bit patterns.
//   k_tv_decide      one block per problem: thread 0 takes the decision, all threads copy the winner's points and flags out.
// Every output word is written by these kernels, so nothing has to be preset.
#include "common.h"
#include "two_view.h"
#include "orb_stage.h"
#include "ransac_stage.h"
#include <cmath>
#include <vector>

namespace osh {

constexpr int kTvWave = 64;
constexpr int kTvBlock = 256;   // k_tv_check_rt, k_tv_decide

struct TvView {
  const TvProblem* prob;
  const float2* pt1; const float2* pt2; const float2* pn1; const float2* pn2;   // [matches of the batch]
  const int* sets;                                                              // [iterations of the batch][8]
  float* mn; float* m; float* minv; float* score;   // per (problem, model, iteration): 2 * base_h + model * n_iter + it
  unsigned char* inl;                               // [matches]: the inliers of the branch's model
  float* hx3d; unsigned char* hcode; unsigned* hkey;   // per (problem, motion hypothesis, match): 8 * base_m + hyp * n_matches + i
  TvHead* head;
  unsigned char* out_inlier; unsigned char* out_tri; float* out_x3d;
};

// grid = (max iterations, 2, n_problems)
__global__ __launch_bounds__(kTvWave) void k_tv_hypothesis(TvView v) {
#pragma clang fp contract(off)
  const TvProblem& P = v.prob[blockIdx.z];
  const int it = blockIdx.x, model = blockIdx.y, lane = threadIdx.x;
  if (it >= P.n_iter) return;
  const int n = P.n_matches;
  const int* set = v.sets + 8 * ((size_t)P.base_h + it);
  double row[9];
  if (lane < kTvRows) {
    const int j = model == 0 ? lane >> 1 : (lane < 8 ? lane : 0);
    const size_t m = (size_t)P.base_m + set[j];
    const float2 a = v.pn1[m], b = v.pn2[m];
    float r[9];
    tv_system_row(model, lane, a.x, a.y, b.x, b.y, r);
#pragma unroll
    for (int k = 0; k < 9; ++k) row[k] = (double)r[k];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) row[k] = lane - kTvRows == k ? 1.0 : 0.0;   // V; lanes 25..63 carry zeros
  }
  const double mine = null_vector_wave<9, kJacobiSweeps>(row, 9);
  float h[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = (float)__shfl(mine, kTvRows + k);

  float T2x[9], Mn[9], M[9], Minv[9];
  if (model == 0) tv_inverse3(P.T2, T2x); else tv_transpose3(P.T2, T2x);
  tv_model(model, h, T2x, P.T1, Mn, M, Minv);
  const size_t g = 2 * (size_t)P.base_h + (size_t)model * P.n_iter + it;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) { v.mn[9 * g + k] = Mn[k]; v.m[9 * g + k] = M[k]; v.minv[9 * g + k] = Minv[k]; }
  }
  const float invSigmaSquare = tv_inv_sigma_square(P.sigma);
  __shared__ float2 terms[kTvWave];
  float score = 0.f;
  for (int base = 0; base < n; base += kTvWave) {
    const int i = base + lane;
    float t1 = 0.f, t2 = 0.f;
    if (i < n) {
      const float2 a = v.pt1[(size_t)P.base_m + i], b = v.pt2[(size_t)P.base_m + i];
      tv_check(model, M, Minv, invSigmaSquare, a.x, a.y, b.x, b.y, t1, t2);
    }
    terms[lane] = make_float2(t1, t2);
    __syncthreads();
    const int cnt = min(kTvWave, n - base);
    for (int k = 0; k < cnt; ++k) { const float2 t = terms[k]; score = score + t.x; score = score + t.y; }   // match order
    __syncthreads();
  }
  if (lane == 0) v.score[g] = score;
}

// grid = n_problems
__global__ __launch_bounds__(kTvWave) void k_tv_select(TvView v) {
#pragma clang fp contract(off)
  const TvProblem& P = v.prob[blockIdx.x];
  const int lane = threadIdx.x, n = P.n_matches;
  TvHead& H = v.head[blockIdx.x];
  __shared__ float s_score[kTvWave];
  __shared__ int s_idx[kTvWave];
  __shared__ int s_branch;
  __shared__ float s_m[9], s_minv[9];
  for (int model = 0; model < 2; ++model) {
    const size_t g0 = 2 * (size_t)P.base_h + (size_t)model * P.n_iter;
    float best = 0.f;
    int idx = -1;
    for (int it = lane; it < P.n_iter; it += kTvWave) {
      const float sc = v.score[g0 + it];
      if (sc > best) { best = sc; idx = it; }
    }
    s_score[lane] = best; s_idx[lane] = idx;
    __syncthreads();
    if (lane == 0) {
      if (model == 0) tv_head_clear(H);
      float b = 0.f;
      int bi = -1;
      for (int l = 0; l < kTvWave; ++l)
        if (s_idx[l] >= 0 && (bi < 0 || s_score[l] > b || (s_score[l] == b && s_idx[l] < bi))) { b = s_score[l]; bi = s_idx[l]; }
      if (model == 0) { H.sh = b; H.best_h = bi; } else { H.sf = b; H.best_f = bi; }
      if (bi >= 0)
        for (int k = 0; k < 9; ++k) (model == 0 ? H.H21 : H.F21)[k] = v.m[9 * (g0 + bi) + k];
    }
    __syncthreads();
  }
  if (lane == 0) {
    tv_choose_branch(H);
    s_branch = H.branch;
    if (H.branch >= 0) {
      const size_t g = 2 * (size_t)P.base_h + (H.branch == 1 ? (size_t)H.best_h : (size_t)P.n_iter + H.best_f);
      for (int k = 0; k < 9; ++k) { s_m[k] = v.m[9 * g + k]; s_minv[k] = v.minv[9 * g + k]; }
    }
  }
  __syncthreads();
  const int branch = s_branch;
  int count = 0;
  if (branch >= 0) {
    float M[9], Minv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { M[k] = s_m[k]; Minv[k] = s_minv[k]; }
    const float invSigmaSquare = tv_inv_sigma_square(P.sigma);
    for (int base = 0; base < n; base += kTvWave) {
      const int i = base + lane;
      bool in = false;
      if (i < n) {
        const float2 a = v.pt1[(size_t)P.base_m + i], b = v.pt2[(size_t)P.base_m + i];
        float t1, t2;
        in = tv_check(branch == 1 ? 0 : 1, M, Minv, invSigmaSquare, a.x, a.y, b.x, b.y, t1, t2);
        v.inl[(size_t)P.base_m + i] = in ? 1 : 0;
      }
      count += __popcll(__ballot(in));
    }
  } else {
    for (int i = lane; i < n; i += kTvWave) v.inl[(size_t)P.base_m + i] = 0;
  }
  if (lane == 0 && branch >= 0) {
    H.n_inliers = count;
    tv_motion(P.K, H);
  }
}

// grid = (8, n_problems)
__global__ __launch_bounds__(kTvBlock) void k_tv_check_rt(TvView v) {
#pragma clang fp contract(off)
  const TvProblem& P = v.prob[blockIdx.y];
  TvHead& H = v.head[blockIdx.y];
  const int hyp = blockIdx.x, tid = threadIdx.x, n = P.n_matches;
  if (hyp >= H.n_hyp) return;   // n_good and parallax of the slot are 0 since tv_head_clear
  __shared__ int s_good;
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_k;
  if (tid == 0) s_good = 0;
  __syncthreads();
  float K[9], R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) { K[k] = P.K[k]; R[k] = H.R[hyp][k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = H.t[hyp][k];
  TvCamera2 cam;
  tv_camera2(K, R, t, cam);
  const float th2 = tv_th2(P.sigma);
  const size_t g0 = 8 * (size_t)P.base_m + (size_t)hyp * n;
  for (int i = tid; i < n; i += kTvBlock) {
    int code = 0;
    unsigned key = 0xFFFFFFFFu;
    float x[3] = {0.f, 0.f, 0.f}, cosp = 0.f;
    if (v.inl[(size_t)P.base_m + i]) {
      const float2 a = v.pt1[(size_t)P.base_m + i], b = v.pt2[(size_t)P.base_m + i];
      code = tv_check_rt(K, R, t, cam, th2, a.x, a.y, b.x, b.y, x, cosp);
      if (code) { key = tv_cos_key(cosp); atomicAdd(&s_good, 1); }
    }
    v.hcode[g0 + i] = (unsigned char)code; v.hkey[g0 + i] = key;
    v.hx3d[3 * (g0 + i)] = x[0]; v.hx3d[3 * (g0 + i) + 1] = x[1]; v.hx3d[3 * (g0 + i) + 2] = x[2];
  }
  __syncthreads();
  const int nGood = s_good;
  if (nGood == 0) return;   // the same for every thread
  // the key of rank min(50, nGood - 1) among the counted matches: a thread reads back only what it wrote above
  if (tid == 0) { s_prefix = 0; s_k = min(50, nGood - 1); }
  unsigned mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    for (int i = tid; i < n; i += kTvBlock)
      if (v.hcode[g0 + i] && (v.hkey[g0 + i] & mask) == prefix) atomicAdd(&s_hist[(v.hkey[g0 + i] >> shift) & 255u], 1u);
    __syncthreads();
    if (tid == 0) {
      int k = s_k;
      unsigned b = 0;
      while (b < 255u && (unsigned)k >= s_hist[b]) { k -= (int)s_hist[b]; ++b; }
      s_k = k; s_prefix = prefix | (b << shift);
    }
    mask |= 255u << shift;
    __syncthreads();
  }
  if (tid == 0) { H.n_good[hyp] = nGood; H.parallax[hyp] = tv_parallax(tv_key_cos(s_prefix)); }
}

// grid = n_problems
__global__ __launch_bounds__(kTvBlock) void k_tv_decide(TvView v) {
  const TvProblem& P = v.prob[blockIdx.x];
  TvHead& H = v.head[blockIdx.x];
  const int tid = threadIdx.x, n = P.n_matches;
  __shared__ int s_winner;
  if (tid == 0) { tv_finish(H); s_winner = H.winner; }
  __syncthreads();
  const int winner = s_winner;
  const size_t g0 = 8 * (size_t)P.base_m + (size_t)(winner < 0 ? 0 : winner) * n;
  for (int i = tid; i < n; i += kTvBlock) {
    const size_t o = (size_t)P.base_m + i;
    const int code = winner >= 0 ? v.hcode[g0 + i] : 0;
    v.out_inlier[o] = v.inl[o];
    v.out_tri[o] = code == 2;
#pragma unroll
    for (int k = 0; k < 3; ++k) v.out_x3d[3 * o + k] = code ? v.hx3d[3 * (g0 + i) + k] : 0.f;
  }
}

struct TwoViewState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
};

static bool tv_all_finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
  return true;
}

static int tv_validate(int n_problems, const osh_two_view_problem* ps, RansacBatch& batch) {
  if (n_problems > OSH_TWOVIEW_MAX_PROBLEMS) { set_error("osh_orb_two_view_reconstruct: more than %d problems", OSH_TWOVIEW_MAX_PROBLEMS); return OSH_ERR_UNSUPPORTED; }
  batch.base.reserve((size_t)n_problems);
  for (int k = 0; k < n_problems; ++k) {
    const osh_two_view_problem& p = ps[k];
    if (p.n_matches < 0 || p.n_iterations < 0 || p.n_keys1 < 0 || p.n_keys2 < 0) { set_error("problem %d: negative count", k); return OSH_ERR_INVALID; }
    if (p.n_matches > OSH_TWOVIEW_MAX_MATCHES) { set_error("problem %d: more than %d matches", k, OSH_TWOVIEW_MAX_MATCHES); return OSH_ERR_UNSUPPORTED; }
    if (p.n_iterations > OSH_TWOVIEW_MAX_ITERATIONS) { set_error("problem %d: more than %d iterations", k, OSH_TWOVIEW_MAX_ITERATIONS); return OSH_ERR_UNSUPPORTED; }
    batch.add(p.n_matches, p.n_iterations, 0);
    if (batch.N > (size_t)OSH_TWOVIEW_MAX_TOTAL_MATCHES) { set_error("osh_orb_two_view_reconstruct: more than %d matches in one call", OSH_TWOVIEW_MAX_TOTAL_MATCHES); return OSH_ERR_UNSUPPORTED; }
    if (batch.I > (size_t)OSH_TWOVIEW_MAX_TOTAL_ITERATIONS) { set_error("osh_orb_two_view_reconstruct: more than %d iterations in one call", OSH_TWOVIEW_MAX_TOTAL_ITERATIONS); return OSH_ERR_UNSUPPORTED; }
    if (!tv_all_finite(p.K, 9) || !tv_all_finite(p.T1, 9) || !tv_all_finite(p.T2, 9) || !std::isfinite(p.sigma)) { set_error("problem %d: K, T1, T2 or sigma not finite", k); return OSH_ERR_INVALID; }
    if (p.K[0] == 0.f || p.K[4] == 0.f) { set_error("problem %d: fx or fy is 0", k); return OSH_ERR_INVALID; }
    if (p.sigma == 0.f) { set_error("problem %d: sigma is 0", k); return OSH_ERR_INVALID; }
    const size_t n = (size_t)p.n_matches;
    if (n && (!p.idx1 || !p.idx2 || !p.pt1 || !p.pt2 || !p.pn1 || !p.pn2)) { set_error("problem %d: NULL match array with n_matches = %d", k, p.n_matches); return OSH_ERR_INVALID; }
    if (!tv_all_finite(p.pt1, n * 2) || !tv_all_finite(p.pt2, n * 2)) { set_error("problem %d: keypoint coordinate not finite", k); return OSH_ERR_INVALID; }
    if (!tv_all_finite(p.pn1, n * 2) || !tv_all_finite(p.pn2, n * 2)) { set_error("problem %d: normalised coordinate not finite", k); return OSH_ERR_INVALID; }
    for (size_t i = 0; i < n; ++i) {
      if (p.idx1[i] < 0 || p.idx1[i] >= p.n_keys1) { set_error("problem %d: match %zu: index %d outside [0, %d) of frame 1", k, i, p.idx1[i], p.n_keys1); return OSH_ERR_INVALID; }
      if (p.idx2[i] < 0 || p.idx2[i] >= p.n_keys2) { set_error("problem %d: match %zu: index %d outside [0, %d) of frame 2", k, i, p.idx2[i], p.n_keys2); return OSH_ERR_INVALID; }
    }
    OSH_TRY(validate_minimal_sets<8>("osh_orb_two_view_reconstruct", k, p.sets, p.n_iterations, p.n_matches, "matches"));
  }
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_two_view_reconstruct(osh_orb_ctx* c, int32_t n_problems, const osh_two_view_problem* ps, const osh_two_view_result* results) {
  PhaseClock clock;
  if (n_problems < 0 || (n_problems && (!ps || !results))) { set_error("osh_orb_two_view_reconstruct: bad arguments"); return OSH_ERR_INVALID; }
  RansacBatch batch;
  OSH_TRY(tv_validate(n_problems, ps, batch));   // the problems first: a refusal needs no context and no device
  if (!c) { set_error("osh_orb_two_view_reconstruct: no context"); return OSH_ERR_INVALID; }
  if (n_problems == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  TwoViewState* st = orb_state<TwoViewState>(c, kOrbAttachTwoView);
  clock.profiling = orb_profiling(c);
  bool debug = false;
  for (int k = 0; k < n_problems; ++k) debug = debug || results[k].debug_model_n || results[k].debug_model || results[k].debug_score;

  const size_t nP = (size_t)n_problems, M = batch.N, I = batch.I;
  Layout in, out, work;
  const auto s_prob = in.take<TvProblem>(nP);
  const auto s_pt1 = in.take<float2>(M); const auto s_pt2 = in.take<float2>(M);
  const auto s_pn1 = in.take<float2>(M); const auto s_pn2 = in.take<float2>(M);
  const auto s_sets = in.take<int>(I * 8);
  const auto o_head = out.take<TvHead>(nP);
  const auto o_inl = out.take<unsigned char>(M); const auto o_tri = out.take<unsigned char>(M);
  const auto o_x3d = out.take<float>(M * 3);
  // the per-iteration models and scores are results only when a caller asks for the debug arrays; otherwise they stay on the device
  Layout& hyp = debug ? out : work;
  const auto h_mn = hyp.take<float>(I * 18); const auto h_m = hyp.take<float>(I * 18); const auto h_score = hyp.take<float>(I * 2);
  const auto w_minv = work.take<float>(I * 18);
  const auto w_inl = work.take<unsigned char>(M);
  const auto w_x3d = work.take<float>(M * 24); const auto w_code = work.take<unsigned char>(M * 8); const auto w_key = work.take<unsigned>(M * 8);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  for (int k = 0; k < n_problems; ++k) {
    const osh_two_view_problem& p = ps[k];
    const size_t n = (size_t)p.n_matches, bm = batch.base[k].p;
    tv_fill_problem(s_prob.in(h)[k], p, (int)bm, (int)batch.base[k].h);
    if (n) {
      std::memcpy(s_pt1.in(h) + bm, p.pt1, n * 8); std::memcpy(s_pt2.in(h) + bm, p.pt2, n * 8);
      std::memcpy(s_pn1.in(h) + bm, p.pn1, n * 8); std::memcpy(s_pn2.in(h) + bm, p.pn2, n * 8);
    }
  }
  batch.stage_sets<8>(s_sets.in(h), ps);
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  char* dw = st->call.dev_work();
  char* dh = debug ? dout : dw;
  TvView v{};
  v.prob = s_prob.in(di);
  v.pt1 = s_pt1.in(di); v.pt2 = s_pt2.in(di); v.pn1 = s_pn1.in(di); v.pn2 = s_pn2.in(di); v.sets = s_sets.in(di);
  v.mn = h_mn.in(dh); v.m = h_m.in(dh); v.score = h_score.in(dh); v.minv = w_minv.in(dw);
  v.inl = w_inl.in(dw); v.hx3d = w_x3d.in(dw); v.hcode = w_code.in(dw); v.hkey = w_key.in(dw);
  v.head = o_head.in(dout); v.out_inlier = o_inl.in(dout); v.out_tri = o_tri.in(dout); v.out_x3d = o_x3d.in(dout);
  if (batch.max_iter > 0) {
    hipLaunchKernelGGL(k_tv_hypothesis, dim3((unsigned)batch.max_iter, 2, (unsigned)n_problems), dim3(kTvWave), 0, s, v);
    OSH_TRY(launch_check("two-view hypotheses"));
  }
  hipLaunchKernelGGL(k_tv_select, dim3((unsigned)n_problems), dim3(kTvWave), 0, s, v);
  OSH_TRY(launch_check("two-view selection"));
  hipLaunchKernelGGL(k_tv_check_rt, dim3(8, (unsigned)n_problems), dim3(kTvBlock), 0, s, v);
  OSH_TRY(launch_check("two-view CheckRT"));
  hipLaunchKernelGGL(k_tv_decide, dim3((unsigned)n_problems), dim3(kTvBlock), 0, s, v);
  OSH_TRY(launch_check("two-view decision"));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_problems; ++k) {
    const osh_two_view_result& r = results[k];
    const size_t n = (size_t)ps[k].n_matches, ni = (size_t)ps[k].n_iterations, bm = batch.base[k].p, bh = batch.base[k].h;
    tv_write_head(r, o_head.in(ho)[k]);
    scatter(r.inlier, o_inl, ho, bm, n); scatter(r.triangulated, o_tri, ho, bm, n); scatter(r.x3d, o_x3d, ho, bm, n, 3);
    if (debug) {
      scatter(r.debug_model_n, h_mn, ho, 2 * bh, 2 * ni, 9); scatter(r.debug_model, h_m, ho, 2 * bh, 2 * ni, 9);
      scatter(r.debug_score, h_score, ho, 2 * bh, 2 * ni);
    }
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_two_view_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<TwoViewState>("osh_orb_two_view_get_times", c, kOrbAttachTwoView, ms);
}
