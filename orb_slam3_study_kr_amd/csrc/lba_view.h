// lba_view.h -- what every local-BA kernel sees: constants, controller state, the batch by value, block-wide reductions and the
// dynamic-LDS layouts of the landmark-major kernels (kernel pointers and host byte counts from one description).  DESIGN.md section 25.
#pragma once
#include "common.h"
#include "lba_math.h"
#include "schur_plan.h"
#include "lba_pack.h"

namespace osh {
constexpr int kPoseRec = 21;       // staged pose: quaternion + translation (7), camera (5), rotation matrix (9)
constexpr int kLdsPoses = 512;     // windows with more poses read them from global memory in the landmark-major kernels
constexpr int kMaxDynamicLds = 160 * 1024 - 64;   // bytes of dynamic LDS the kernels of this file opt in to
constexpr int kPasses = kChunkMaxEdges / kChunkEdges;   // passes of 256 edges of a landmark-major block

struct LmState {
  double lambda, ni, currentChi, iniChi, tempChi, rho, scale_pose, chi2_initial;
  int iter;           // index of the running solve() call
  int qmax;           // trials of the running iteration
  int nBad;
  int active;         // window still inside optimize()
  int need_lin;       // next round opens a new iteration (linearise at cur)
  int lin_now;        // this round opened an iteration: the pose side of the linearisation belongs to it
  int need_dl;        // lambda changed since the landmark factors were formed (first lambda, rejected trial)
  int sel;            // state buffer holding the current estimates
  int last_eval_sel;  // buffer whose errors computeActiveErrors saw last
  int iterations;     // cjIterations
  int trials;
  int solve_ok;
  int stop;           // host stop flag snapshot
  int n_trace;
  double chi2_trace[OSH_LBA_MAX_TRACE];
  double lambda_trace[OSH_LBA_MAX_TRACE];
  int trials_trace[OSH_LBA_MAX_TRACE];
};

// Everything the kernels need, passed by value.
struct BatchView {
  int n_windows, n_chunks, n_fposes;
  const WinDesc* win;
  LmState* lm;
  const Chunk* chunks;
  const int* fpose_win;      // [n_fposes] window of each optimisable pose
  // state: [2] buffers
  double* pose_state[2];     // [NP*7]
  double* pt_state[2];       // [NL*3]
  const double* pose_cam;    // [NP*5]
  // sorted edges (landmark-major, poses ascending inside a landmark, free poses first)
  const int* e_pose;         // [NE] window-local pose index
  const int* e_point;        // [NE] window-local landmark index
  const unsigned char* e_kind;   // [NE] sorted-edge kind (kKind*); the pinhole kernels read the sign of e_rec[.][3] instead
  const double* e_rec;       // [NE*4] u v u_right +-invSigma2 of every sorted edge: one 32-byte record (sign bit set = mono)
  const float4* e_rec32;     // the same records as the float32 values they were uploaded as (null unless every record is exact in
                             // float32): the landmark-major kernels are bandwidth bound and read these, 16 bytes an edge
  const double* e_rec2;      // [NE*4] right-camera observation of a fisheye-rig edge (u v - invSigma2), rig batches only
  const int* e_orig;         // [NE] index in the caller's edge order
  const int* e_orig2;        // [NE] caller index of the merged right-camera edge or -1, rig batches only
  const int* lm_off;         // per window L+1 offsets (window-local edge index)
  // Schur plan (schur_plan.h)
  const SItem* sitems;       // [n_items] symmetric items first
  const SRec* srecs;         // landmark records of the items
  const int* spair;          // [n_items*64] contribution index of pose pair (sa,sb) or -1
  const int* scslot;         // [n_items*8] rhs contribution index of row pose sa or -1
  const int* sposex;         // [n_items*8] window-local row pose of slot sa or -1
  const int* sposey;         // [n_items*8] window-local column pose of slot sb or -1
  const I2* pose_crange;     // [NFP] {first, count} of the pose's (item, pose) contributions
  double* hcontrib;          // [n_ccontrib*27] per linearisation: upper(Hpp) (21) + b_p (6) of one item and pose
  double* chi_lin;           // [n_chunks] robust chi2 partial of each chunk at the linearisation point
  double* dmax_lin;          // [n_chunks] largest Hll diagonal entry of the chunk
  const RBlk* rblk;          // [n_rblk] blocks of S + rhs segments with their contribution ranges
  int n_rblk;
  int* pose_lo;              // [NFP] first block row with a non-zero in block column p of the window's S (its column envelope), k_schur_env
  double* contrib;           // [n_contrib*36] per trial: 6x6 products of one item and pose pair
  double* ccontrib;          // [n_ccontrib*6] per trial: rhs products of one item and pose
  // system
  double* Hll;               // [NL*6] upper: 00 01 02 11 12 22
  double* bl;                // [NL*3]
  double* DL;                // [NL*9] landmark factor F (6) + F^T b_l (3), see landmark_factor()
  double* Hpp;               // [NFP*36]
  double* bp;                // [NFP*6]
  double* S;                 // per window (6P)^2, upper triangle valid
  double* bs;                // [NFP*6]
  double* xp;                // [NFP*6]
  double* chi_part;          // [n_chunks] robust chi2 partial of each chunk at the trial estimates (k_backsub)
  double* scale_part;        // [n_chunks]
  double* dmax_pose;         // [NFP]
  int* n_active;             // [1]
  // outputs
  double* out_chi2;          // [NOUT] caller order
  unsigned char* out_depth;  // [NOUT]
};

// Read-only snapshot of the controller fields a kernel needs, taken once at kernel entry (a reference into
// global memory would be re-read after every store: the compiler cannot prove the stores do not alias it).
struct LmView { double lambda; int active, need_lin, lin_now, need_dl, iter, sel, solve_ok, last_eval_sel, iterations; };
__device__ __forceinline__ LmView lm_view(const LmState* lm, int w) {
  const LmState& s = lm[w];
  return LmView{s.lambda, s.active, s.need_lin, s.lin_now, s.need_dl, s.iter, s.sel, s.solve_ok, s.last_eval_sel, s.iterations};
}

// --------------------------------------------------------------------------------------------
// block-wide deterministic reductions (4 wavefronts of 64)
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* sh4) {
  v = dev::wave_sum(v);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh4[wv] = v;
  __syncthreads();
  const double r = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ double block_max(double v, double* sh4) {
  v = dev::wave_max(v);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh4[wv] = v;
  __syncthreads();
  const double r = fmax(fmax(sh4[0], sh4[1]), fmax(sh4[2], sh4[3]));
  __syncthreads();
  return r;
}

// Ordering point for the single-wavefront kernels (64-thread blocks): LDS operations of one wavefront execute in order, so
// only the compiler has to be told not to move LDS accesses across this point.  __syncthreads() would additionally wait for
// every outstanding GLOBAL access of the wavefront (it is also a workgroup-scope memory fence).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Dynamic LDS of the landmark-major kernels, in doubles.  The kernel takes its pointers and the host its byte count from the same
// description (a launch whose budget was worked out apart from the kernel's carve-up once failed: tests/test_gpu_solve.py).
// k_lin_lm: [9 * 256] partials of the ordered sum, [4] reduce scratch, [256 * 3] the chunk's landmarks, the staged poses
struct LinLds {
  static constexpr int kPart = 0, kRed = kPart + 9 * kChunkEdges, kX = kRed + 4, kPose = kX + 3 * kBlock;
  __host__ __device__ static constexpr int doubles(int n_staged) { return kPose + n_staged * kPoseRec; }
};

// k_finalize: the chunk's landmarks of the state evaluated last and of the final state ([256 * 3] each), the staged poses of the
// state evaluated last, then quaternion + translation (7) of every pose of the final state.  The second landmark array and the final
// poses are only filled when the two states differ (a window whose last trial was rejected).
struct FinLds {
  static constexpr int kX = 0, kXf = kX + 3 * kBlock, kPose = kXf + 3 * kBlock;
  __host__ __device__ static constexpr int doubles(int n_staged) { return kPose + n_staged * (kPoseRec + 7); }
};
static_assert(FinLds::doubles(kLdsPoses) * (int)sizeof(double) <= kMaxDynamicLds, "kLdsPoses keyframes of both states fit the block");

// k_backsub for a window of P optimisable and F fixed keyframes: partials, reduce scratch and the chunk's landmarks;
// when `staged`, x_p and the optimisable poses at the current estimates; the trial poses of all keyframes when there are at most
// kLdsPoses.  x_p and the current poses are staged when that fits the block (with two fixed keyframes: up to 393 optimisable ones; the
// budget was once taken for granted up to kLdsPoses, and the launch of a window of 394 to 510 failed); otherwise the kernel reads them
// from global memory, as it does beyond kLdsPoses.
struct BacksubLds {
  static constexpr int kPart = 0, kRed = kPart + 3 * kChunkEdges, kX = kRed + 4, kXp = kX + 3 * kBlock;
  int pose, pose_t, doubles;   // current poses (after x_p), trial poses, the end
  bool staged_t;               // the trial poses of all keyframes are staged
  __host__ __device__ static constexpr BacksubLds of(int P, int F, bool staged) {
    const int pose = kXp + (staged ? 6 * P : 0), pose_t = pose + (staged ? P * kPoseRec : 0);
    const bool staged_t = P + F <= kLdsPoses;
    return BacksubLds{pose, pose_t, pose_t + (staged_t ? (P + F) * kPoseRec : 0), staged_t};
  }
};
__host__ __device__ constexpr int backsub_lds_doubles(int P, int F, bool staged) { return BacksubLds::of(P, F, staged).doubles; }
__host__ __device__ constexpr bool backsub_stages(int P, int F) {
  return P <= kLdsPoses && backsub_lds_doubles(P, F, true) * (int)sizeof(double) <= kMaxDynamicLds;
}
static_assert(backsub_stages(50, 10) && backsub_lds_doubles(50, 10, true) == 4150, "the headline window stages everything");
static_assert(backsub_stages(394, 0) && backsub_lds_doubles(394, 0, true) == 20452, "the largest window that stages x_p and its poses");
static_assert(!backsub_stages(395, 0) && backsub_lds_doubles(395, 0, true) == 20500 && backsub_lds_doubles(395, 0, false) == 9835, "one more does not fit");
static_assert(backsub_stages(6, 506) && backsub_lds_doubles(6, 506, true) == 12454, "kLdsPoses keyframes: the trial poses are staged");
static_assert(backsub_stages(6, 507) && backsub_lds_doubles(6, 507, true) == 1702, "one more: the trial poses stay in global memory");
}  // namespace osh
