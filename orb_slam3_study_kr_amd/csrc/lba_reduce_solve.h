// lba_reduce_solve.h -- after the Schur items of a trial and around the rounds: k_schur_reduce / _deep, k_pose_reduce, k_solve,
// k_big_finish, the controller k_control, and k_schur_env, k_reset, k_set_stop.  DESIGN.md section 25.
#pragma once
#include <cfloat>
#include "lba_view.h"
#include "ldlt_block.h"
#include "big_solve.h"
#include "g2o_lm.h"

namespace osh {
// --------------------------------------------------------------------------------------------
// k_schur_reduce: S(i,j) = [i == j] (Hpp_i + lambda I) - sum of the block's contributions,
// b_s(i) = b_p(i) - sum of the pose's rhs contributions; every entry by one thread, contributions in plan order.
// --------------------------------------------------------------------------------------------
// k_schur_reduce (calls of more than 8 windows, about six contributions per block).  With one thread per entry a lane reads 8 bytes
// per load, and 8-byte loads stream at 0.54-0.70 of the rate of 16-byte ones: that kernel ran at 4.0 of 6.3 TB/s however many loads
// it kept in flight.  Here a lane owns two neighbouring entries of a block (18 lanes per block, 14 blocks per 256 threads, 16-byte
// loads and stores, two sums side by side).  The envelope, the initial value and the first eight contributions are requested before
// one wait; the loads a block does not have are skipped (immediate offsets from one address: a load costs its compare and itself; the
// wait that follows a load a lane may skip is a wait for every load of the wavefront, so everything the block needs from its RBlk
// entry and its window is worked out before the first of them).  Every entry is still v = init; v -= c_0; v -= c_1; ... in plan
// order by one thread.  Several blocks per 18-lane group (RBlk entries and window state requested together) only cost wavefronts
// per CU: DESIGN.md section 4.

// contributions k .. k + 7 of a block of n, as far as it has them: this lane's two entries of each
__device__ __forceinline__ void reduce_load8(double2* t, const double* c, int k, int n) {
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (k + u < n) t[u] = *reinterpret_cast<const double2*>(c + (size_t)k * 36 + u * 36);
}

__global__ __launch_bounds__(256) void k_schur_reduce(BatchView bv) {
  const int t = threadIdx.x / 18, e = threadIdx.x - 18 * t;
  const int idx = blockIdx.x * 14 + t;
  if (t >= 14 || idx >= bv.n_rblk) return;
  const int r = e / 3, cc = 2 * (e - 3 * r);   // entries (r, cc) and (r, cc + 1) of the block: 16 bytes, 16-byte aligned in every array
  // No early exit below: one would let the compiler put the loads behind it, one round trip after the other.  What the lane has to
  // do is kept as indices, -1: nothing.
  const RBlk rb = bv.rblk[idx];
  const WinDesc& wd = bv.win[rb.win];
  const LmState& st = bv.lm[rb.win];
  const int fpose_off = wd.fpose_off, n = wd.n;
  const long long S_off = wd.S_off;
  const double lambda = st.lambda;
  const bool live = st.active != 0;
  const int i = rb.ij & 0xffff, j = (rb.ij >> 16) & 0xffff;
  const bool rhs = j == 0xffff;
  const long long gp = (long long)fpose_off + i;
  const int cnt = live && !rhs ? rb.count : 0;
  const long long off = (long long)rb.start * 36 + 2 * e;                                                   // the block's first contribution
  const long long src = live && i == j ? gp * 36 + 2 * e : -1;                                              // a diagonal block: its entries of Hpp
  const long long dst = live && !rhs ? S_off + (long long)(6 * i + r) * n + 6 * j + cc : -1;                // where the entries go in S
  const long long seg = live && rhs && e < 3 ? gp * 6 + 2 * e : -1;                                         // a rhs segment: its entries of b_p and b_s
  // the block column's entry of pose_lo, read by every lane (a lane that may skip it would wait for it on the spot: the compiler
  // moves the comparison to the load); without an envelope any int of an optimisable pose, not looked at
  const int lo = (bv.pose_lo ? bv.pose_lo : bv.fpose_win)[live && !rhs ? fpose_off + j : 0];
  double2 init{0.0, 0.0}, tt[8];
  if (src >= 0) init = *reinterpret_cast<const double2*>(bv.Hpp + src);
  reduce_load8(tt, bv.contrib + off, 0, cnt);
  __builtin_amdgcn_sched_barrier(0);
  double ax = 0.0, ay = 0.0;
  if (src >= 0) { ax = init.x + ((r == cc) ? lambda : 0.0); ay = init.y + ((r == cc + 1) ? lambda : 0.0); }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (u < cnt) { ax -= tt[u].x; ay -= tt[u].y; }
  for (int k = 8; k < cnt; k += 8) {   // a block with more than eight contributions: eight more in flight at a time
    double2 more[8];
    reduce_load8(more, bv.contrib + off, k, cnt);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k + u < cnt) { ax -= more[u].x; ay -= more[u].y; }
  }
  // A block above the column envelope of S (no landmark joins keyframe i to j or to any keyframe before i, k_schur_env) is zero, is
  // never touched by the envelope factorisation of k_solve and was zeroed at upload: nothing to write (it has no contributions either).
  if (dst >= 0 && (!bv.pose_lo || i >= lo)) *reinterpret_cast<double2*>(bv.S + dst) = double2{ax, ay};
  if (seg >= 0) {   // a rhs segment (P of a window's P (P + 1) / 2 + P entries): three lanes, eight contributions in flight
    double2 a = *reinterpret_cast<const double2*>(bv.bp + seg);
    const double* c = bv.ccontrib + (size_t)rb.start * 6 + 2 * e;
    int k = 0;
    for (; k + 8 <= rb.count; k += 8) {
      double2 t8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t8[u] = *reinterpret_cast<const double2*>(c + (size_t)(k + u) * 6);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 8; ++u) { a.x -= t8[u].x; a.y -= t8[u].y; }
    }
    for (; k < rb.count; ++k) { const double2 t1 = *reinterpret_cast<const double2*>(c + (size_t)k * 6); a.x -= t1.x; a.y -= t1.y; }
    *reinterpret_cast<double2*>(bv.bs + seg) = a;
  }
}

// k_schur_reduce_deep (calls of at most 8 windows): one block of S per 36-lane group, 24 contributions in flight where a block has
// that many -- a call with few windows cuts its Schur items small (item_max_lm) and has four times as many contributions per block.
__global__ __launch_bounds__(256) void k_schur_reduce_deep(BatchView bv) {
  const int t = threadIdx.x / 36, el = threadIdx.x - 36 * t;
  const int idx = blockIdx.x * 7 + t;
  if (t >= 7 || idx >= bv.n_rblk) return;
  const RBlk rb = bv.rblk[idx];
  const WinDesc wd = bv.win[rb.win];   // by value: the fields stay in SGPRs across the kernel's stores
  const LmView st = lm_view(bv.lm, rb.win);
  if (!st.active) return;
  const int i = rb.ij & 0xffff, j = (rb.ij >> 16) & 0xffff;
  if (j == 0xffff) {
    if (el >= 6) return;
    const size_t gp = (size_t)wd.fpose_off + i;
    double v = bv.bp[gp * 6 + el];
    const double* c = bv.ccontrib + (size_t)rb.start * 6 + el;
    int k = 0;
    for (; k + 24 <= rb.count; k += 24) {
      double t[24];
#pragma unroll
      for (int u = 0; u < 24; ++u) t[u] = c[(size_t)(k + u) * 6];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 24; ++u) v -= t[u];
    }
    for (; k + 8 <= rb.count; k += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = c[(size_t)(k + u) * 6];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 8; ++u) v -= t[u];
    }
    for (; k < rb.count; ++k) v -= c[(size_t)k * 6];
    bv.bs[gp * 6 + el] = v;
    return;
  }
  // A block above the column envelope of S (no landmark joins keyframe i to j or to any keyframe before i, k_schur_env) is zero, is
  // never touched by the envelope factorisation of k_solve and was zeroed at upload: nothing to write.
  if (bv.pose_lo && i < bv.pose_lo[wd.fpose_off + j]) return;
  const int r = el / 6, cc = el - 6 * r;
  double v = 0.0;
  if (i == j) v = bv.Hpp[((size_t)wd.fpose_off + i) * 36 + el] + ((r == cc) ? st.lambda : 0.0);
  const double* c = bv.contrib + (size_t)rb.start * 36 + el;
  int k = 0;
  for (; k + 24 <= rb.count; k += 24) {
    double t[24];
#pragma unroll
    for (int u = 0; u < 24; ++u) t[u] = c[(size_t)(k + u) * 36];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 24; ++u) v -= t[u];
  }
  for (; k + 8 <= rb.count; k += 8) {   // eight contributions in flight (one load per iteration left every memory round trip exposed),
    double t[8];                        // subtracted in plan order: the sum is the same number as before
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = c[(size_t)(k + u) * 36];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) v -= t[u];
  }
  for (; k < rb.count; ++k) v -= c[(size_t)k * 36];
  bv.S[wd.S_off + (size_t)(6 * i + r) * wd.n + 6 * j + cc] = v;
}

// k_pose_reduce: Hpp_i (full symmetric 6x6), b_p(i) and the largest diagonal entry of pose i from the item
// contributions, in plan order.  32 lanes per optimisable pose: lane k < 27 sums entry k of the contributions
// (one contribution = 27 contiguous doubles -> coalesced, the loads of successive contributions are independent).
// mode as in k_schur_fused: 0 = the first round of optimize(), 1 = rounds that opened a later iteration.
__global__ __launch_bounds__(64) void k_pose_reduce(BatchView bv, int mode) {
  const int gp = blockIdx.x * 2 + (threadIdx.x >> 5);
  const int k = threadIdx.x & 31;
  if (gp >= bv.n_fposes) return;
  const int w = bv.fpose_win[gp];
  const LmView st = lm_view(bv.lm, w);
  if (!st.active || !(mode == 0 ? st.need_lin != 0 : (st.lin_now != 0 && st.iter > 0))) return;
  const I2 rg = bv.pose_crange[gp];
  double a = 0.0;
  if (k < 27) {
    const double* src = bv.hcontrib + (size_t)rg.x * 27 + k;
    int c = 0;
    for (; c + 16 <= rg.y; c += 16) {   // sixteen contributions in flight (a single window cut into small items has ~100 per pose), added in plan order
      double t[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) t[u] = src[(size_t)(c + u) * 27];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 16; ++u) a += t[u];
    }
    for (; c + 4 <= rg.y; c += 4) {
      const double v0 = src[(size_t)c * 27], v1 = src[(size_t)(c + 1) * 27], v2 = src[(size_t)(c + 2) * 27], v3 = src[(size_t)(c + 3) * 27];
      a += v0; a += v1; a += v2; a += v3;
    }
    for (; c < rg.y; ++c) a += src[(size_t)c * 27];
    if (k < 21) {
      // entry k of the upper triangle -> (r, cc)
      int r = 0, rem = k;
      while (rem >= 6 - r) { rem -= 6 - r; ++r; }
      const int cc = r + rem;
      double* Ho = bv.Hpp + (size_t)gp * 36;
      Ho[r * 6 + cc] = a;
      Ho[cc * 6 + r] = a;
    } else {
      bv.bp[(size_t)gp * 6 + (k - 21)] = a;
    }
  }
  // largest diagonal entry: upper-triangle entries 0, 6, 11, 15, 18, 20 are the diagonal
  __shared__ double shd[64];
  shd[threadIdx.x] = fabs(a);
  wave_sync();
  if (k == 0) {
    const double* d = shd + (threadIdx.x & 32);
    bv.dmax_pose[gp] = fmax(fmax(fmax(d[0], d[6]), fmax(d[11], d[15])), fmax(d[18], d[20]));
  }
}

// Tail of the reduced-system solve of one window: x_p out, pose update T <- exp(x) T into the trial buffer and the pose part of
// computeScale.  `xs`: the solution (n doubles, LDS or global), `shw`: NT/64 doubles of LDS scratch.
template <int NT>
__device__ void solve_tail(BatchView& bv, const WinDesc& wd, LmState& st, const double* xs, double* shw, bool ok) {
  const int tid = threadIdx.x, n = wd.n;
  double* xp = bv.xp + (size_t)wd.fpose_off * 6;
  for (int k = tid; k < n; k += NT) xp[k] = xs[k];   // zeros when the factorisation failed
  __syncthreads();
  const int cur = st.sel, tr_sel = st.sel ^ 1;
  const double lambda = st.lambda;
  double sc = 0.0;
  for (int i = tid; i < wd.P; i += NT) {
    double u[6], qin[7], qout[7];
#pragma unroll
    for (int k = 0; k < 6; ++k) u[k] = xs[6 * i + k];
#pragma unroll
    for (int k = 0; k < 7; ++k) qin[k] = bv.pose_state[cur][((size_t)wd.pose_off + i) * 7 + k];
    dev::pose_oplus(u, qin, qout);
#pragma unroll
    for (int k = 0; k < 7; ++k) bv.pose_state[tr_sel][((size_t)wd.pose_off + i) * 7 + k] = qout[k];
    const double* bpi = bv.bp + ((size_t)wd.fpose_off + i) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) sc += u[k] * (lambda * u[k] + bpi[k]);
  }
  sc = dev::wave_sum(sc);
  if ((tid & 63) == 0) shw[tid >> 6] = sc;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int k = 0; k < NT / 64; ++k) tot += shw[k];
    st.scale_pose = tot; st.solve_ok = ok ? 1 : 0;
  }
}

// --------------------------------------------------------------------------------------------
// k_solve: dense blocked LDL^T (no pivoting, upper storage) of the reduced camera system of
// one window per block, forward elimination fused (rhs carried as an extra column), blocked
// back-substitution, then the pose update T <- exp(x) T and the pose part of computeScale.
// LDS: one panel [nb][W] (unscaled rows), x [n], d [nb] (ldlt_block.h); which instantiation runs: solve_plan.h.
// --------------------------------------------------------------------------------------------
template <int NB, int NT>
__global__ __launch_bounds__(NT) void k_solve(BatchView bv, int W) {
  constexpr int kSolveThreads = NT;
  extern __shared__ __attribute__((aligned(16))) double sh[];   // all LDS scratch is dynamic (16-B aligned base)
  const int w = blockIdx.x;
  const WinDesc& wd = bv.win[w];
  LmState& st = bv.lm[w];
  if (!st.active) return;
  const int n = wd.n;
  double* A = bv.S + wd.S_off;
  double* rhs = bv.bs + (size_t)wd.fpose_off * 6;
  double *xs, *shw;
  const bool ok = ldlt_solve_block<NB, kSolveThreads>(A, rhs, n, W, sh, xs, shw, bv.pose_lo ? bv.pose_lo + wd.fpose_off : nullptr);
  solve_tail<kSolveThreads>(bv, wd, st, xs, shw, ok);
}

// One reduced system too large for the LDS-resident factorisation (global BA of a long session): big_solve.h has factored and
// solved it in global memory, the solution sits in the window's `bs`; this is the tail of k_solve for that window.
__global__ __launch_bounds__(256) void k_big_finish(BatchView bv, int w, const int* fail) {
  __shared__ double shw[8];
  const WinDesc& wd = bv.win[w];
  LmState& st = bv.lm[w];
  if (!st.active) return;
  double* x = bv.bs + (size_t)wd.fpose_off * 6;
  const bool ok = *fail == 0;
  if (!ok) {
    for (int k = threadIdx.x; k < wd.n; k += 256) x[k] = 0.0;    // zeros when the factorisation failed
    __syncthreads();
  }
  solve_tail<256>(bv, wd, st, x, shw, ok);
}

// --------------------------------------------------------------------------------------------
// k_control: one wavefront per window.
//   phase 0 (after the landmark side of a linearisation): open the iteration (currentChi, lambda init).
//   phase 1 (after the trial residual): gain ratio, accept / reject, stop rules.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_control(BatchView bv, int phase) {
  const int w = blockIdx.x;
  const WinDesc& wd = bv.win[w];
  LmState& st = bv.lm[w];
  const int lane = threadIdx.x;
  // the count of active windows is taken by phase 1; phase 0 of the same round (an earlier launch, no increments of its own) clears it
  // (a hipMemsetAsync per round was a 4.4 us fill kernel of its own: 2 % of a single window's optimize())
  if (phase == 0 && w == 0 && lane == 0) *bv.n_active = 0;
  if (!st.active) return;
  // robust chi2 of the state evaluated last = sum of the partials (fixed order): chunk partials of k_lin_lm after a
  // linearisation, of k_backsub after a trial
  double chi = 0.0;
  if (phase == 0) { for (int c = lane; c < wd.n_chunks; c += 64) chi += bv.chi_lin[wd.chunk_off + c]; }
  else { for (int c = lane; c < wd.n_chunks; c += 64) chi += bv.chi_part[wd.chunk_off + c]; }
  chi = dev::wave_sum(chi);
  if (phase == 0) {
    if (!st.need_lin) return;
    double dm = 0.0;
    if (st.iter == 0) {
      for (int c = lane; c < wd.n_chunks; c += 64) dm = fmax(dm, bv.dmax_lin[wd.chunk_off + c]);
      for (int p = lane; p < wd.P; p += 64) dm = fmax(dm, bv.dmax_pose[wd.fpose_off + p]);
      dm = dev::wave_max(dm);
    }
    if (lane == 0) {
      st.currentChi = chi; st.tempChi = chi; st.iniChi = chi;
      if (st.iter == 0) {
        st.chi2_initial = chi;
        st.lambda = (wd.lambda_init > 0) ? wd.lambda_init : kLmTau * dm;  // computeLambdaInit
        st.ni = 2.0; st.nBad = 0;
        st.need_dl = 1;   // the landmark factors could not be formed before lambda was known
      }
      st.rho = 0.0; st.qmax = 0; st.need_lin = 0; st.lin_now = 1;
      st.last_eval_sel = st.sel;
    }
    return;
  }
  // ---- phase 1
  double sc = 0.0;
  for (int c = lane; c < wd.n_chunks; c += 64) sc += bv.scale_part[wd.chunk_off + c];
  sc = dev::wave_sum(sc);
  if (lane != 0) return;
  double tempChi = chi;
  if (!st.solve_ok) tempChi = DBL_MAX;
  st.tempChi = tempChi;
  st.last_eval_sel = st.sel ^ 1;  // computeActiveErrors just ran on the trial estimates
  st.lin_now = 0;
  const LmTrial trial = lm_judge_trial(st.lambda, st.ni, st.currentChi, tempChi, st.scale_pose + sc);
  const double rho = trial.rho;
  if (trial.accepted) {
    st.currentChi = tempChi;
    st.sel ^= 1;  // discardTop: the trial estimates become current (pop: a rejected trial's buffer is simply abandoned)
  }
  st.rho = rho;
  st.qmax++;
  st.trials++;
  const bool again = (rho < 0) && (st.qmax < kLmMaxTrials) && !st.stop;
  st.need_dl = again ? 1 : 0;   // another trial of this iteration: same Hll, new lambda
  if (!again) {
    // the iteration is over
    st.iterations++;
    if (st.n_trace < OSH_LBA_MAX_TRACE) {
      st.chi2_trace[st.n_trace] = st.currentChi;
      st.lambda_trace[st.n_trace] = st.lambda;
      st.trials_trace[st.n_trace] = st.qmax;
      st.n_trace++;
    }
    const bool ok = lm_iteration_goes_on(st.nBad, st.iniChi, st.currentChi, st.qmax, rho);
    st.iter++;
    if (!ok || st.iter >= wd.max_iter || st.stop) st.active = 0;
    else st.need_lin = 1;
  }
  if (st.active) atomicAdd(bv.n_active, 1);
}

// Column envelope of every window's reduced system, once per upload: block (i, j) of S is structurally non-zero when a landmark is
// seen by both keyframes, i.e. when the plan gave it a contribution (RBlk::count > 0); the diagonal always is (Hpp + lambda I).
// pose_lo[j] = smallest such i.  The factorisation of k_solve keeps this envelope and skips the tile columns outside it (ldlt_block.h).
__global__ __launch_bounds__(256) void k_schur_env(BatchView bv) {
  __shared__ int sh_off[4];
  const int w = blockIdx.x, tid = threadIdx.x;
  const WinDesc wd = bv.win[w];
  int off = 0;
  for (int k = tid; k < w; k += 256) { const int Pk = bv.win[k].P; off += Pk * (Pk + 1) / 2 + Pk; }
  for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
  if ((tid & 63) == 0) sh_off[tid >> 6] = off;
  __syncthreads();
  const int base = sh_off[0] + sh_off[1] + sh_off[2] + sh_off[3];
  const int P = wd.P;
  for (int j = tid; j < P; j += 256) {
    int lo = j;
    for (int i = 0; i < j; ++i) {
      if (bv.rblk[base + i * P - i * (i - 1) / 2 + (j - i)].count > 0) { lo = i; break; }
    }
    bv.pose_lo[wd.fpose_off + j] = lo;
  }
}

// reset the controller before optimize()  (the host counts the windows this leaves active itself, from the same three conditions:
// reset_state; *n_active is cleared by phase 0 and counted by phase 1 of every round)
__global__ void k_reset(BatchView bv, const unsigned char* stop) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= bv.n_windows) return;
  const WinDesc& wd = bv.win[w];
  LmState& st = bv.lm[w];
  st.lambda = -1.0; st.ni = 2.0; st.currentChi = 0; st.iniChi = 0; st.tempChi = 0; st.rho = 0; st.scale_pose = 0;
  st.chi2_initial = 0;
  st.iter = 0; st.qmax = 0; st.nBad = 0;
  st.stop = stop ? stop[w] : 0;
  st.active = (wd.max_iter > 0 && !st.stop && wd.E > 0) ? 1 : 0;
  st.need_lin = st.active; st.lin_now = 0; st.need_dl = 0;
  st.sel = 0; st.last_eval_sel = 0; st.iterations = 0; st.trials = 0; st.solve_ok = 1; st.n_trace = 0;
}

__global__ void k_set_stop(BatchView bv, const unsigned char* stop) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= bv.n_windows) return;
  bv.lm[w].stop = stop[w];
}
}  // namespace osh
