// lba_device.hip -- local bundle adjustment on MI355X (gfx950): HIP kernels + C-ABI driver.
//
// Replaces, for a batch of independent windows, what
//   optimizer.initializeOptimization(); optimizer.optimize(10);     src/Optimizer.cc:1410-1411
// does on one CPU thread in the reference (g2o LM + Schur block solver).  See
// DESIGN.md for the data layout and the roofline of each kernel.
//
// Kernel map (reference loop -> kernel), "g2o/" = Thirdparty/g2o/g2o/:
//   k_lin_lm      computeActiveErrors + activeRobustChi2 + the landmark side of buildSystem
//                 g2o/core/sparse_optimizer.cpp:61-114, block_solver.hpp:502-560,
//                 base_binary_edge.hpp:55-120  (Hll, b_l) + setLambda / D->inverse() of every landmark
//                 (block_solver.hpp:389,582-587) as the factor F, F F^T = (Hll + lambda I)^-1
//   k_schur_fused the pose side of buildSystem (per-item Hpp / b_p partials) and BlockSolver::solve's Schur
//                 part, block_solver.hpp:367-439: landmarks grouped by observer set (schur_plan.h), one
//                 wavefront per group, (B F)(B F)^T on the FP64 matrix cores.  The 6x3 blocks Hpl are formed
//                 in registers from the edge description (lba_math.h) and never stored
//   k_pose_reduce Hpp, b_p from the group partials, fixed order
//   k_schur_reduce  S = Hpp + lambda I - sum of the group products, b_s = b_p - ..., fixed order
//   k_solve       LinearSolverEigen::solve -> dense blocked LDL^T, g2o/solvers/linear_solver_eigen.h:94-124,
//                 + pose update (VertexSE3Expmap::oplusImpl)
//   k_backsub     landmark back-substitution block_solver.hpp:461-483 + VertexSBAPointXYZ::oplusImpl
//                 + computeScale partials (optimization_algorithm_levenberg.cpp:187-194)
//                 + computeActiveErrors / activeRobustChi2 at the trial estimates (the trial residual, a kernel of its own
//                 until round 3)
//   k_control     the Levenberg-Marquardt controller, optimization_algorithm_levenberg.cpp:61-169,
//                 and the optimize() loop conditions, sparse_optimizer.cpp:354-419
//   k_finalize    per-edge chi2 / isDepthPositive for the outlier test, src/Optimizer.cc:1413-1460
// The kernels live in headers by role (lba_view.h, lba_chunk.h and the three below: DESIGN.md section 25); this file keeps the
// context, the launch sequence and the C-ABI.
#include <cstdlib>
#include <cstdio>
#include <atomic>
#include <chrono>
#include <thread>
#include "lba_lm_kernels.h"
#include "lba_schur_items.h"
#include "lba_reduce_solve.h"
#include "solve_plan.h"
#include "lba_pack_device.h"
#include <algorithm>
#include <cstring>
#include <vector>

// =============================================================================================
// Host driver
// =============================================================================================
using namespace osh;

namespace osh {

constexpr int kDevicePackMinWindows = 24;   // smaller batches are packed by host threads (osh_lba_upload)

// Final estimates in the caller's order, contiguous per batch, so that the download is a handful of large copies:
// optimisable poses of every window (the state buffer the controller ended on) and the landmarks with the upload's
// renumbering undone.
__global__ __launch_bounds__(256) void k_gather_out(BatchView bv, const int* lm_perm, int n_points_total, double* out_pose, double* out_pts,
                                                    const int* pt_win) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_points_total) {
    const int w = pt_win[t];
    const WinDesc& wd = bv.win[w];
    const int sel = bv.lm[w].sel;
    const int jn = t - wd.pt_off;
    const size_t dst = (size_t)wd.pt_off + lm_perm[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_pts[dst * 3 + k] = bv.pt_state[sel][(size_t)(wd.pt_off + jn) * 3 + k];
  }
  if (t < bv.n_fposes) {
    const int w = bv.fpose_win[t];
    const WinDesc& wd = bv.win[w];
    const int sel = bv.lm[w].sel;
    const int i = t - wd.fpose_off;
#pragma unroll
    for (int k = 0; k < 7; ++k) out_pose[(size_t)t * 7 + k] = bv.pose_state[sel][((size_t)wd.pose_off + i) * 7 + k];
  }
}

// float32 observation records -> the 32-byte records the kernels read (lba_pack.h: rec_f32)
__global__ __launch_bounds__(256) void k_widen_rec(const float4* src, double* dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 v = src[i];
  double2* d = reinterpret_cast<double2*>(dst + i * 4);
  d[0] = make_double2((double)v.x, (double)v.y);
  d[1] = make_double2((double)v.z, (double)v.w);
}

}  // namespace osh

struct osh_lba_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  void* attach[kAttachCount] = {};
  void (*attach_free[kAttachCount])(void*) = {};
  KernelTimer timer;
  // host-side batch description
  int n_windows = 0;
  PackedBatch pb;
  std::vector<const volatile unsigned char*> stop_ptr;
  bool any_stop = false;
  int solve_nb = 24, solve_W = 0, solve_threads = kSolveThreadsLatency;
  bool solve_big = false;            // a window's reduced system exceeds the LDS-resident factorisation: big_solve.h
  DevBuf d_bigV, d_bigz, d_bigfail;
  size_t solve_lds = 0, backsub_lds = 0, lin_lds = 0, fin_lds = 0;
  double upload_pack_ms = 0, upload_copy_ms = 0;
  // edge kernels of the batch's camera models: the KannalaBrandt8 instantiations only when a window asks for them
  void (*kp_lin_lm)(BatchView) = nullptr;
  void (*kp_schur_sym)(BatchView, int, int) = nullptr;
  void (*kp_schur_cross)(BatchView, int, int) = nullptr;
  void (*kp_pose_only)(BatchView, int, int) = nullptr;   // the pose side alone (first round of optimize(), launched with mode 0)
  void (*kp_finalize)(BatchView) = nullptr;
  void (*kp_backsub)(BatchView) = nullptr;
  void (*kp_debug_hpl)(BatchView, double*) = nullptr;
  // staging + device buffers
  PinBuf h_arena[2], h_out;
  DevBuf d_arena[2], d_ptwin, d_erec;
  DevBuf d_lm, d_pose[2], d_pt[2], d_hcontrib, d_chi_lin, d_dmax_lin, d_contrib, d_ccontrib;
  DevBuf d_Hll, d_bl, d_DL, d_Hpp, d_bp, d_S, d_bs, d_xp, d_chi, d_scale, d_dmaxp, d_nactive, d_out_chi2, d_out_depth, d_stop;
  DevBuf d_out_pose, d_out_pts, d_dbg, d_pose_lo;
  int* h_nactive = nullptr;          // pinned
  unsigned char* h_stop = nullptr;   // pinned [n_windows]
  size_t h_stop_cap = 0;
  BatchView bv{};
  bool optimized = false;
  DevPackState dpack;                // lba_pack_device.hip: the packer on the device
  int pack_mode = -1;                // -1: device unless the batch needs the host packer / the environment says otherwise; 0 device; 1 host
  bool device_packed = false;        // the last upload's arenas exist on the device only (pb.arena[] are null)
  template <class T> T* dsec(int s) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(d_arena[pb.sec_arena(s)].p) + pb.sec_off(s)); }
};

extern "C" int osh_lba_create(int device, osh_lba_ctx** out) {
  if (!out) { set_error("osh_lba_create: out is NULL"); return OSH_ERR_INVALID; }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device visible"); return OSH_ERR_NO_DEVICE; }
  if (device < 0 || device >= n) { set_error("device %d out of range (have %d)", device, n); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(device));
  osh_lba_ctx* c = new osh_lba_ctx();
  c->device = device;
  OSH_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  OSH_HIP(hipHostMalloc((void**)&c->h_nactive, sizeof(int)));
  zero_new_host(c->h_nactive, sizeof(int));
  *out = c;
  return OSH_OK;
}

int osh::lba_stream(osh_lba_ctx* c, int* device, hipStream_t* stream) {
  if (!c) { set_error("null context"); return OSH_ERR_INVALID; }
  *device = c->device; *stream = c->stream;
  OSH_HIP(hipSetDevice(c->device));
  return OSH_OK;
}

// Attachments are created on first use and released by osh_lba_destroy -- not by a thread_local destructor at process exit,
// when the HIP runtime may already be gone.
void** osh::lba_attachment(osh_lba_ctx* c, LbaAttachSlot slot, void (*free_fn)(void*)) {
  if (!c || slot < 0 || slot >= kAttachCount) return nullptr;
  c->attach_free[slot] = free_fn;
  return &c->attach[slot];
}

extern "C" void osh_lba_destroy(osh_lba_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (int k = 0; k < kAttachCount; ++k) if (c->attach[k] && c->attach_free[k]) { c->attach_free[k](c->attach[k]); c->attach[k] = nullptr; }
  c->timer.destroy();
  c->dpack.release_events();
  if (c->h_nactive) (void)hipHostFree(c->h_nactive);
  if (c->h_stop) (void)hipHostFree(c->h_stop);
  hipStream_t s = c->stream;
  delete c;   // DevBuf / PinBuf members release their memory
  if (s) (void)hipStreamDestroy(s);
}

extern "C" int osh_lba_upload(osh_lba_ctx* c, int32_t nw, const osh_lba_problem* pr) {
  if (!c || nw <= 0 || !pr) { set_error("osh_lba_upload: bad arguments"); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(c->device));
  OSH_HIP(hipStreamSynchronize(c->stream));
  c->optimized = false;
  c->n_windows = 0;                  // stays 0 (nothing uploaded) unless this upload completes
  c->stop_ptr.assign(nw, nullptr);
  c->any_stop = false;
  for (int w = 0; w < nw; ++w) { c->stop_ptr[w] = pr[w].stop_flag; if (pr[w].stop_flag) c->any_stop = true; }

  // ---- packing: on the device (lba_pack_device.hip) from the caller's arrays in the caller's order, or -- a handful of windows,
  // OSH_LBA_PACK=host -- by host threads straight into pinned staging (lba_pack.h) and one copy per arena
  const auto t0 = std::chrono::steady_clock::now();
  PackedBatch& pb = c->pb;
  hipStream_t s = c->stream;
  // Default rule: batches go to the device packer (one thread block per window: 512 windows pack in 6 ms of kernels against 65 ms of
  // 16 host threads); a handful of windows stay on the host, where one thread packs a 50-keyframe window in 1.3 ms -- below the
  // latency of three one-block kernels and two round trips (1.9 ms, profiles/pack_device.py).
  bool on_device = device_pack_supported(nw, pr);
  if (c->pack_mode >= 0) on_device = on_device && c->pack_mode == 0;
  else if (const char* e = std::getenv("OSH_LBA_PACK")) on_device = on_device && std::strcmp(e, "host") != 0;
  else on_device = on_device && nw >= kDevicePackMinWindows;
  c->device_packed = on_device;
  const PackCuts cuts = pack_cuts(nw);   // the environment is read here, once per upload
  if (on_device) {
    const int rc = device_pack_batch(c->dpack, s, nw, pr, default_pack_threads(nw), cuts, pb, c->d_arena, c->d_ptwin);
    if (rc != OSH_OK) { set_error("%s", pb.msg); return rc; }
  } else {
    const int rc = pack_batch(nw, pr, [&](int which, size_t bytes) { return c->h_arena[which].reserve(bytes); }, default_pack_threads(nw), cuts, pb);
    if (rc != OSH_OK) { set_error("%s", pb.msg); return rc; }
  }
  const auto t1 = std::chrono::steady_clock::now();
  if (!on_device) {
    for (int a = 0; a < 2; ++a) {
      OSH_TRY(c->d_arena[a].reserve(pb.arena_bytes[a]));
      OSH_HIP(hipMemcpyAsync(c->d_arena[a].p, pb.arena[a], pb.arena_bytes[a], hipMemcpyHostToDevice, s));
    }
  }
  const size_t NP = pb.NP, NFP = pb.NFP, NL = pb.NL, NOUT = pb.NOUT;

  // ---- LDS budgets
  {
    c->lin_lds = (size_t)LinLds::doubles(std::min(pb.np_max, kLdsPoses)) * sizeof(double);
    c->fin_lds = (size_t)FinLds::doubles(std::min(pb.np_max, kLdsPoses)) * sizeof(double);
    int backsub_doubles = 0;   // the largest need of a window (backsub_lds_doubles: each window stages what fits)
    for (const WinDesc& d : pb.win) backsub_doubles = std::max(backsub_doubles, backsub_lds_doubles(d.P, d.F, backsub_stages(d.P, d.F)));
    c->backsub_lds = (size_t)backsub_doubles * sizeof(double);
    // One block per window with the widest panel that fits.  A batch takes 256-thread blocks: the one LDS panel of ldlt_block.h
    // (70 KB for 50 keyframes) lets two windows share a CU, and the factorisation is latency bound, so they overlap (measured:
    // 5.5 ms of solve per 512-window step against 6.0 with 512-thread blocks, profiles/solve_sweep.sh); a few windows take 512 threads.
    // (the rule, its limits and the three measurement switches: solve_plan.h)
    auto knob = [](const char* name) { const char* e = std::getenv(name); return e ? std::atoi(e) : 0; };
    const SolvePlan plan = lba_solve_plan(pb.n_max, nw, knob("OSH_LBA_SOLVE_NB"), knob("OSH_LBA_SOLVE_THREADS"), knob("OSH_LBA_SOLVE_BIG"));
    c->solve_threads = plan.threads;
    c->solve_big = plan.big;
    if (c->solve_big) {
      // beyond 438 optimisable poses (global BA of a long session; OSH_LBA_SOLVE_BIG=1: whatever the size) the system is factored in
      // global memory, one window at a time
      if (pb.n_max / 6 > kBigMaxPoses) {
        set_error("window with %d optimisable poses: the dense reduced system is limited to %d poses", pb.n_max / 6, kBigMaxPoses);
        return OSH_ERR_UNSUPPORTED;
      }
      OSH_TRY(c->d_bigV.reserve(std::max<size_t>((size_t)kBigNB * pb.n_max * 8, 8))); OSH_TRY(c->d_bigz.reserve(std::max<size_t>((size_t)pb.n_max * 8, 8)));
      OSH_TRY(c->d_bigfail.reserve(sizeof(int)));
    }
    c->solve_nb = plan.nb;
    c->solve_W = ldlt_row_stride(pb.n_max);
    c->solve_lds = plan.lds_bytes;
  }

  // ---- work buffers
  auto R = [&](DevBuf& b, size_t bytes) { return b.reserve(std::max<size_t>(bytes, 8)); };
  OSH_TRY(R(c->d_lm, nw * sizeof(LmState)));
  for (int k = 0; k < 2; ++k) { OSH_TRY(R(c->d_pose[k], NP * 7 * 8)); OSH_TRY(R(c->d_pt[k], NL * 3 * 8)); }
  OSH_TRY(R(c->d_contrib, pb.n_contrib * 36 * 8)); OSH_TRY(R(c->d_ccontrib, pb.n_ccontrib * 6 * 8));
  OSH_TRY(R(c->d_hcontrib, pb.n_ccontrib * 27 * 8)); OSH_TRY(R(c->d_chi_lin, pb.n_chunks * 8)); OSH_TRY(R(c->d_dmax_lin, pb.n_chunks * 8));
  OSH_TRY(R(c->d_Hll, NL * 6 * 8)); OSH_TRY(R(c->d_bl, NL * 3 * 8)); OSH_TRY(R(c->d_DL, NL * 9 * 8));
  OSH_TRY(R(c->d_Hpp, NFP * 36 * 8)); OSH_TRY(R(c->d_bp, NFP * 6 * 8)); OSH_TRY(R(c->d_S, pb.S_total * 8));
  OSH_TRY(R(c->d_bs, NFP * 6 * 8)); OSH_TRY(R(c->d_xp, NFP * 6 * 8));
  OSH_TRY(R(c->d_chi, pb.n_chunks * 8)); OSH_TRY(R(c->d_scale, pb.n_chunks * 8));
  OSH_TRY(R(c->d_dmaxp, NFP * 8)); OSH_TRY(R(c->d_nactive, sizeof(int)));
  OSH_TRY(R(c->d_out_chi2, NOUT * 8)); OSH_TRY(R(c->d_out_depth, NOUT)); OSH_TRY(R(c->d_stop, nw));
  OSH_TRY(R(c->d_out_pose, NFP * 7 * 8)); OSH_TRY(R(c->d_out_pts, NL * 3 * 8)); OSH_TRY(R(c->d_ptwin, NL * 4)); OSH_TRY(R(c->d_pose_lo, NFP * 4));
  if (c->h_stop_cap < (size_t)nw) {
    if (c->h_stop) (void)hipHostFree(c->h_stop);
    OSH_HIP(hipHostMalloc((void**)&c->h_stop, nw));
    zero_new_host(c->h_stop, nw);
    c->h_stop_cap = nw;
  }
  OSH_HIP(hipMemsetAsync(c->d_xp.p, 0, std::max<size_t>(NFP * 6 * 8, 8), s));
  // state buffer 1: the fixed keyframes' poses, which no kernel writes, once per upload (reset_state has the whole argument; the
  // optimisable poses copied with them are overwritten before they are read)
  if (NP) OSH_HIP(hipMemcpyAsync(c->d_pose[1].p, c->dsec<double>(PackedBatch::POSE), NP * 7 * 8, hipMemcpyDeviceToDevice, s));
  if (!on_device) {
    // window of every landmark (for k_gather_out): the host packer writes it into the tail of the pinned output staging (reused
    // by the download later); the device packer has filled d_ptwin itself
    int* h_ptwin = static_cast<int*>(c->h_out.reserve(std::max<size_t>(NL * 4, 8)));
    if (!h_ptwin) { set_error("cannot allocate pinned staging"); return OSH_ERR_DEVICE; }
    for (int w = 0; w < nw; ++w) std::fill(h_ptwin + pb.win[w].pt_off, h_ptwin + pb.win[w].pt_off + pb.win[w].L, w);
    if (NL) OSH_HIP(hipMemcpyAsync(c->d_ptwin.p, h_ptwin, NL * 4, hipMemcpyHostToDevice, s));
  }

  BatchView& bv = c->bv;
  bv.n_windows = nw; bv.n_chunks = (int)pb.n_chunks; bv.n_fposes = (int)NFP;
  bv.win = c->dsec<WinDesc>(PackedBatch::WIN); bv.lm = c->d_lm.as<LmState>(); bv.chunks = c->dsec<Chunk>(PackedBatch::CHUNKS);
  bv.fpose_win = c->dsec<int>(PackedBatch::FPW);
  for (int k = 0; k < 2; ++k) { bv.pose_state[k] = c->d_pose[k].as<double>(); bv.pt_state[k] = c->d_pt[k].as<double>(); }
  bv.pose_cam = c->dsec<double>(PackedBatch::CAM);
  bv.e_pose = c->dsec<int>(PackedBatch::EPOSE); bv.e_point = c->dsec<int>(PackedBatch::EPOINT);
  bv.e_kind = c->dsec<unsigned char>(PackedBatch::EKIND);
  bv.e_rec = c->dsec<double>(PackedBatch::EREC); bv.e_rec2 = c->dsec<double>(PackedBatch::EREC2);
  if (pb.rec_f32) {
    OSH_TRY(R(c->d_erec, pb.NE * 32));
    if (pb.NE) {
      hipLaunchKernelGGL(k_widen_rec, dim3((unsigned)((pb.NE + 255) / 256)), dim3(256), 0, s, c->dsec<float4>(PackedBatch::EREC), c->d_erec.as<double>(), pb.NE);
      OSH_TRY(launch_check("k_widen_rec"));
    }
    bv.e_rec = c->d_erec.as<double>();
  }
  bv.e_rec32 = (pb.rec_f32 && !std::getenv("OSH_LBA_NO_F32_RECORDS")) ? c->dsec<float4>(PackedBatch::EREC) : nullptr;
  bv.e_orig = c->dsec<int>(PackedBatch::EORIG); bv.e_orig2 = c->dsec<int>(PackedBatch::EORIG2);
  bv.lm_off = c->dsec<int>(PackedBatch::LMOFF);
  bv.sitems = c->dsec<SItem>(PackedBatch::ITEMS); bv.srecs = c->dsec<SRec>(PackedBatch::RECS);
  bv.spair = c->dsec<int>(PackedBatch::SPAIR); bv.scslot = c->dsec<int>(PackedBatch::SCSLOT);
  bv.sposex = c->dsec<int>(PackedBatch::POSEX); bv.sposey = c->dsec<int>(PackedBatch::POSEY);
  bv.rblk = c->dsec<RBlk>(PackedBatch::RBLK); bv.n_rblk = (int)pb.n_rblk;
  bv.pose_crange = c->dsec<I2>(PackedBatch::CRANGE);
  bv.contrib = c->d_contrib.as<double>(); bv.ccontrib = c->d_ccontrib.as<double>(); bv.hcontrib = c->d_hcontrib.as<double>();
  bv.chi_lin = c->d_chi_lin.as<double>(); bv.dmax_lin = c->d_dmax_lin.as<double>();
  bv.Hll = c->d_Hll.as<double>(); bv.bl = c->d_bl.as<double>(); bv.DL = c->d_DL.as<double>();
  bv.Hpp = c->d_Hpp.as<double>(); bv.bp = c->d_bp.as<double>(); bv.S = c->d_S.as<double>();
  bv.bs = c->d_bs.as<double>(); bv.xp = c->d_xp.as<double>();
  bv.chi_part = c->d_chi.as<double>(); bv.scale_part = c->d_scale.as<double>();
  bv.dmax_pose = c->d_dmaxp.as<double>();
  bv.n_active = c->d_nactive.as<int>();
  bv.out_chi2 = c->d_out_chi2.as<double>(); bv.out_depth = c->d_out_depth.as<unsigned char>();
  bv.pose_lo = c->d_pose_lo.as<int>();
  hipLaunchKernelGGL(k_schur_env, dim3((unsigned)nw), dim3(256), 0, s, bv);
  OSH_TRY(launch_check("k_schur_env"));
  // dense factorisations (OSH_LBA_DENSE_SOLVE, and big_solve.h for maps beyond the LDS-resident solve) read and fill every block
  if (std::getenv("OSH_LBA_DENSE_SOLVE") || c->solve_big) bv.pose_lo = nullptr;
  else OSH_HIP(hipMemsetAsync(c->d_S.p, 0, std::max<size_t>(pb.S_total * 8, 8), s));   // the blocks above the envelope stay zero from here on
  OSH_HIP(hipStreamSynchronize(s));   // the staging arenas may be rewritten by the next upload
  const auto t2 = std::chrono::steady_clock::now();
  c->upload_pack_ms = on_device ? c->dpack.host_ms : std::chrono::duration<double, std::milli>(t1 - t0).count();
  c->upload_copy_ms = (on_device ? c->dpack.device_ms : 0.0) + std::chrono::duration<double, std::milli>(t2 - t1).count();

  const bool f32 = bv.e_rec32 != nullptr;
  if (pb.has_kb8) {
    c->kp_lin_lm = f32 ? k_lin_lm<true, true> : k_lin_lm<true, false>; c->kp_schur_sym = k_schur_fused<true, true>; c->kp_schur_cross = k_schur_fused<false, true>;
    c->kp_finalize = f32 ? k_finalize<true, true> : k_finalize<true, false>; c->kp_pose_only = k_schur_fused<true, true, false, true>;
    c->kp_backsub = f32 ? k_backsub<true, true> : k_backsub<true, false>; c->kp_debug_hpl = k_debug_hpl<true>;
  } else {
    c->kp_lin_lm = f32 ? k_lin_lm<false, true> : k_lin_lm<false, false>; c->kp_schur_cross = k_schur_fused<false, false>;
    // symmetric items: the diagonal and ragged tiles from 4 x 4 blocks; OSH_LBA_SCHUR_TILES keeps whole tiles (the same bits: tests/test_gpu_schur_blocks.py)
    c->kp_schur_sym = std::getenv("OSH_LBA_SCHUR_TILES") ? k_schur_fused<true, false> : k_schur_fused<true, false, true>;
    c->kp_finalize = f32 ? k_finalize<false, true> : k_finalize<false, false>; c->kp_pose_only = k_schur_fused<true, false, false, true>;
    c->kp_backsub = f32 ? k_backsub<false, true> : k_backsub<false, false>; c->kp_debug_hpl = k_debug_hpl<false>;
  }
  // The controls of tests/test_gpu_lba_pose_only.py, tests/test_gpu_lba_finalize.py and of the before/after traces: the full Schur
  // kernel called with mode 0 for the pose side of the first round, and the edge-by-edge k_finalize (no dynamic LDS).  The same bits.
  if (std::getenv("OSH_LBA_POSE_PASS_FULL")) c->kp_pose_only = c->kp_schur_sym;
  if (std::getenv("OSH_LBA_FINALIZE_PLAIN")) { c->kp_finalize = pb.has_kb8 ? k_finalize_plain<true> : k_finalize_plain<false>; c->fin_lds = 0; }

  // opt in to large dynamic LDS
  constexpr int kTB = kSolveThreadsBatch, kTL = kSolveThreadsLatency;
  OSH_TRY(allow_dynamic_lds(c->device, kMaxDynamicLds, k_solve<24, kTB>, k_solve<12, kTB>, k_solve<6, kTB>, k_solve<24, kTL>,
                            k_solve<12, kTL>, k_solve<6, kTL>, k_backsub<false, false>, k_backsub<false, true>, k_backsub<true, false>,
                            k_backsub<true, true>, k_lin_lm<false, false>, k_lin_lm<false, true>, k_lin_lm<true, false>, k_lin_lm<true, true>,
                            k_finalize<false, false>, k_finalize<false, true>, k_finalize<true, false>, k_finalize<true, true>));
  c->n_windows = nw;
  return OSH_OK;
}

static bool snapshot_stop(osh_lba_ctx* c) {
  bool any = false;
  for (int w = 0; w < c->n_windows; ++w) {
    const volatile unsigned char* f = c->stop_ptr[w];
    c->h_stop[w] = (f && *f) ? 1 : 0;
    any |= c->h_stop[w] != 0;
  }
  return any;
}

#define LAUNCH(kid, name, grid, block, lds, ...)                                              \
  do {                                                                                        \
    if ((grid) > 0) {                                                                         \
      const bool _t = c->timer.begin(kid, s);                                                 \
      hipLaunchKernelGGL(name, dim3((unsigned)(grid)), dim3(block), (lds), s, __VA_ARGS__);   \
      if (_t) c->timer.end(s);                                                                \
      OSH_TRY(launch_check(#name));                                                           \
    }                                                                                         \
  } while (0)

// the instantiation of k_solve chosen at upload time (panel width x threads per block)
static int launch_solve(osh_lba_ctx* c, hipStream_t s) {
  if (c->solve_big) {
    for (int w = 0; w < c->n_windows; ++w) {
      const WinDesc& d = c->pb.win[w];
      if (d.n == 0) continue;
      BigSolve g;
      g.A = c->d_S.as<double>() + d.S_off; g.b = c->d_bs.as<double>() + (size_t)d.fpose_off * 6;
      g.V = c->d_bigV.as<double>(); g.z = c->d_bigz.as<double>(); g.fail = c->d_bigfail.as<int>();
      g.active = &(c->d_lm.as<LmState>() + w)->active;
      g.n = d.n;
      OSH_HIP(hipMemsetAsync(g.fail, 0, sizeof(int), s));
      for (int k0 = 0; k0 < d.n; k0 += kBigNB) {
        hipLaunchKernelGGL(k_big_diag, dim3(1), dim3(64), 0, s, g, k0);
        const int tr = d.n - (k0 + kBigNB);   // trailing rows
        if (tr <= 0) break;
        hipLaunchKernelGGL(k_big_panel, dim3((unsigned)((tr + 255) / 256)), dim3(256), 0, s, g, k0);
        const unsigned T = (unsigned)((tr + kBigTile - 1) / kBigTile);
        hipLaunchKernelGGL(k_big_update, dim3(T, T), dim3(256), 0, s, g, k0);
      }
      hipLaunchKernelGGL(k_big_back, dim3(1), dim3(1024), 0, s, g);
      hipLaunchKernelGGL(k_big_finish, dim3(1), dim3(256), 0, s, c->bv, w, g.fail);
    }
    return launch_check("k_big_solve");
  }
  const dim3 grid((unsigned)c->n_windows);
#define OSH_SOLVE_CASE(NB, NT) \
  if (c->solve_nb == NB && c->solve_threads == NT) hipLaunchKernelGGL((k_solve<NB, NT>), grid, dim3(NT), c->solve_lds, s, c->bv, c->solve_W);
  OSH_SOLVE_CASE(24, kSolveThreadsBatch) OSH_SOLVE_CASE(12, kSolveThreadsBatch) OSH_SOLVE_CASE(6, kSolveThreadsBatch)
  OSH_SOLVE_CASE(24, kSolveThreadsLatency) OSH_SOLVE_CASE(12, kSolveThreadsLatency) OSH_SOLVE_CASE(6, kSolveThreadsLatency)
#undef OSH_SOLVE_CASE
  return launch_check("k_solve");
}

// Back to the uploaded estimates, controller reset.  `*n_active`: the windows k_reset leaves active, counted here from the same
// three conditions (the stream starts the first round without a round trip for a number the host already has).
// State buffer 0 is rewritten whole.  Of buffer 1 every entry but the fixed keyframes' poses is written before it is read:
//   poses of optimisable keyframes   k_solve's tail (solve_tail) writes all P of an active window into buffer sel ^ 1 before
//                                    k_backsub reads them, in every round; sel only becomes 1 by accepting such a trial
//   landmarks                        k_backsub writes every trial landmark of an active window's chunks before its own trial residual
//                                    reads them, and again sel only becomes 1 afterwards
//   a window that is not active      stays at sel == last_eval_sel == 0: k_finalize and k_gather_out read buffer 0 alone
//   poses of fixed keyframes         read from both buffers (the trial residual stages all P + F), written by no kernel: they are in
//                                    buffer 1 since the upload copied the pose array there, and still are
// So nothing is copied into buffer 1 here.  `both` (the debug entries, which read buffer 1 of windows that may not be active)
// restores it as well.
static int reset_state(osh_lba_ctx* c, int* n_active, bool both = false) {
  hipStream_t s = c->stream;
  const PackedBatch& pb = c->pb;
  for (int k = 0; k < (both ? 2 : 1); ++k) {
    if (pb.NP) OSH_HIP(hipMemcpyAsync(c->d_pose[k].p, c->dsec<double>(PackedBatch::POSE), pb.NP * 7 * 8, hipMemcpyDeviceToDevice, s));
    if (pb.NL) OSH_HIP(hipMemcpyAsync(c->d_pt[k].p, c->dsec<double>(PackedBatch::PT), pb.NL * 3 * 8, hipMemcpyDeviceToDevice, s));
  }
  const unsigned char* dstop = nullptr;
  if (c->any_stop) {
    snapshot_stop(c);
    OSH_HIP(hipMemcpyAsync(c->d_stop.p, c->h_stop, c->n_windows, hipMemcpyHostToDevice, s));
    dstop = c->d_stop.as<unsigned char>();
  }
  hipLaunchKernelGGL(k_reset, dim3((c->n_windows + 63) / 64), dim3(64), 0, s, c->bv, dstop);
  OSH_TRY(launch_check("k_reset"));
  int n = 0;
  for (int w = 0; w < c->n_windows; ++w) n += (pb.win[w].max_iter > 0 && !(c->any_stop && c->h_stop[w]) && pb.win[w].E > 0) ? 1 : 0;
  if (n_active) *n_active = n;
  // (a stop flag is polled into the same pinned snapshot after every round: the copy above has to have read it first)
  if (c->any_stop) OSH_HIP(hipStreamSynchronize(s));
  return OSH_OK;
}

static int read_nactive(osh_lba_ctx* c, int* out) {
  OSH_HIP(hipMemcpyAsync(c->h_nactive, c->d_nactive.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  OSH_HIP(hipStreamSynchronize(c->stream));
  *out = *c->h_nactive;
  return OSH_OK;
}

// The first linearisation of optimize(): landmark side, pose side alone (computeLambdaInit needs the diagonal of Hpp before
// any Schur product can be formed), controller phase 0 (lambda), then the landmark factors for that lambda.
static int first_linearisation(osh_lba_ctx* c) {
  hipStream_t s = c->stream;
  const PackedBatch& pb = c->pb;
  LAUNCH(OSH_K_LINEARIZE, c->kp_lin_lm, pb.n_chunks, kBlock, c->lin_lds, c->bv);
  LAUNCH(OSH_K_LIN_POSE, c->kp_pose_only, pb.n_sym, 64, 0, c->bv, 0, 0);
  LAUNCH(OSH_K_POSE_HESS, k_pose_reduce, (pb.NFP + 1) / 2, 64, 0, c->bv, 0);
  LAUNCH(OSH_K_CONTROL, k_control, c->n_windows, 64, 0, c->bv, 0);
  LAUNCH(OSH_K_LIN_AUX, c->kp_lin_lm, pb.n_chunks, kBlock, c->lin_lds, c->bv);
  return OSH_OK;
}

// S and b_s of every active window from the contributions of the trial's Schur items.
static int launch_schur_reduce(osh_lba_ctx* c) {
  hipStream_t s = c->stream;
  const int n = (int)c->pb.n_rblk;
  if (c->n_windows <= 8) { LAUNCH(OSH_K_SCHUR_REDUCE, k_schur_reduce_deep, (n + 6) / 7, 256, 0, c->bv); }
  else { LAUNCH(OSH_K_SCHUR_REDUCE, k_schur_reduce, (n + 13) / 14, 256, 0, c->bv); }
  return OSH_OK;
}

// One LM trial of every active window from the Schur products to the trial residual.
static int trial_kernels(osh_lba_ctx* c, bool later_round) {
  hipStream_t s = c->stream;
  const PackedBatch& pb = c->pb;
  LAUNCH(OSH_K_SCHUR, c->kp_schur_sym, pb.n_sym, 64, 0, c->bv, 0, 1);
  LAUNCH(OSH_K_SCHUR_CROSS, c->kp_schur_cross, pb.n_items - pb.n_sym, 64, 0, c->bv, (int)pb.n_sym, 1);
  if (later_round) LAUNCH(OSH_K_POSE_HESS, k_pose_reduce, (pb.NFP + 1) / 2, 64, 0, c->bv, 1);
  OSH_TRY(launch_schur_reduce(c));
  {
    const bool _t = c->timer.begin(OSH_K_SOLVE, s);
    OSH_TRY(launch_solve(c, s));
    if (_t) c->timer.end(s);
  }
  LAUNCH(OSH_K_BACKSUB, c->kp_backsub, pb.n_chunks, kBlock, c->backsub_lds, c->bv);
  return OSH_OK;
}

extern "C" int osh_lba_optimize(osh_lba_ctx* c) {
  if (!c || c->n_windows <= 0) { set_error("osh_lba_optimize: nothing uploaded"); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const PackedBatch& pb = c->pb;
  if (c->timer.enabled) OSH_TRY(c->timer.init());
  int n_active = 0;
  OSH_TRY(reset_state(c, &n_active));
  int max_iter = 0;
  for (const WinDesc& d : pb.win) max_iter = std::max(max_iter, d.max_iter);
  const long max_rounds = (long)max_iter * kLmMaxTrials + 1;
  for (long round = 0; round < max_rounds && n_active > 0; ++round) {
    if (round == 0) {
      OSH_TRY(first_linearisation(c));
    } else {
      // windows opening an iteration: landmark side + factors; windows repeating a trial: factors for the new lambda
      LAUNCH(OSH_K_LINEARIZE, c->kp_lin_lm, pb.n_chunks, kBlock, c->lin_lds, c->bv);
      LAUNCH(OSH_K_CONTROL, k_control, c->n_windows, 64, 0, c->bv, 0);
    }
    OSH_TRY(trial_kernels(c, round > 0));   // (k_backsub ends with the trial residual of its chunk)
    if (c->any_stop) {
      // terminate() is polled after every trial (levenberg.cpp:149) and before every iteration
      snapshot_stop(c);
      OSH_HIP(hipMemcpyAsync(c->d_stop.p, c->h_stop, c->n_windows, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_set_stop, dim3((c->n_windows + 63) / 64), dim3(64), 0, s, c->bv, c->d_stop.as<unsigned char>());
      OSH_TRY(launch_check("k_set_stop"));
    }
    LAUNCH(OSH_K_CONTROL, k_control, c->n_windows, 64, 0, c->bv, 1);   // (counts the windows still active; cleared by this round's phase 0)
    // A round is one trial; an iteration takes at least one, so no window can finish before `max_iter` rounds unless it converges
    // early -- and every kernel of a round leaves at once for a window that is no longer active.  The first max_iter rounds are
    // therefore queued without waiting for the count of active windows (ten host round trips of an optimize(10) were 0.2 ms of a
    // single window's 2.9 ms); the count is read after them, and after every further round (windows whose trials were rejected).
    // With a stop flag to poll the host looks in after every round, as before.
    if (c->any_stop || round + 1 >= (long)max_iter) {
      OSH_TRY(read_nactive(c, &n_active));
      if (c->timer.enabled) c->timer.collect();
    }
  }
  if (pb.n_chunks) {
    hipLaunchKernelGGL(c->kp_finalize, dim3((unsigned)pb.n_chunks), dim3(kBlock), c->fin_lds, s, c->bv);
    OSH_TRY(launch_check("k_finalize"));
  }
  {
    const size_t n = std::max(pb.NL, pb.NFP);
    if (n) {
      hipLaunchKernelGGL(k_gather_out, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->bv, c->dsec<int>(PackedBatch::LMPERM), (int)pb.NL,
                         c->d_out_pose.as<double>(), c->d_out_pts.as<double>(), c->d_ptwin.as<int>());
      OSH_TRY(launch_check("k_gather_out"));
    }
  }
  OSH_HIP(hipStreamSynchronize(s));
  if (c->timer.enabled) c->timer.collect();
  c->optimized = true;
  return OSH_OK;
}

extern "C" int osh_lba_download(osh_lba_ctx* c, int32_t nw, osh_lba_result* res) {
  if (!c || !res || nw != c->n_windows) { set_error("osh_lba_download: bad arguments"); return OSH_ERR_INVALID; }
  if (!c->optimized) { set_error("osh_lba_download: call osh_lba_optimize first"); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const PackedBatch& pb = c->pb;
  // one pinned staging buffer, five large copies, then per-window memcpy into the caller's arrays
  bool want_pose = false, want_pts = false, want_chi = false, want_depth = false;
  for (int w = 0; w < nw; ++w) { want_pose |= res[w].pose_qt != nullptr; want_pts |= res[w].points != nullptr; want_chi |= res[w].edge_chi2 != nullptr; want_depth |= res[w].edge_depth_pos != nullptr; }
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_lm = 0, o_pose = o_lm + al((size_t)nw * sizeof(LmState)), o_pts = o_pose + al(pb.NFP * 7 * 8), o_chi = o_pts + al(pb.NL * 3 * 8),
               o_depth = o_chi + al(pb.NOUT * 8), total = o_depth + al(pb.NOUT);
  unsigned char* h = static_cast<unsigned char*>(c->h_out.reserve(total));
  if (!h) { set_error("cannot allocate %zu bytes of pinned staging", total); return OSH_ERR_DEVICE; }
  OSH_HIP(hipMemcpyAsync(h + o_lm, c->d_lm.p, (size_t)nw * sizeof(LmState), hipMemcpyDeviceToHost, s));
  if (want_pose && pb.NFP) OSH_HIP(hipMemcpyAsync(h + o_pose, c->d_out_pose.p, pb.NFP * 7 * 8, hipMemcpyDeviceToHost, s));
  if (want_pts && pb.NL) OSH_HIP(hipMemcpyAsync(h + o_pts, c->d_out_pts.p, pb.NL * 3 * 8, hipMemcpyDeviceToHost, s));
  if (want_chi && pb.NOUT) OSH_HIP(hipMemcpyAsync(h + o_chi, c->d_out_chi2.p, pb.NOUT * 8, hipMemcpyDeviceToHost, s));
  if (want_depth && pb.NOUT) OSH_HIP(hipMemcpyAsync(h + o_depth, c->d_out_depth.p, pb.NOUT, hipMemcpyDeviceToHost, s));
  OSH_HIP(hipStreamSynchronize(s));
  const LmState* h_lm = reinterpret_cast<const LmState*>(h + o_lm);
  auto copy_window = [&](int w) {
    const WinDesc& d = pb.win[w];
    const LmState& st = h_lm[w];
    osh_lba_result& r = res[w];
    if (r.pose_qt && d.P) std::memcpy(r.pose_qt, h + o_pose + (size_t)d.fpose_off * 7 * 8, (size_t)d.P * 7 * 8);
    if (r.points && d.L) std::memcpy(r.points, h + o_pts + (size_t)d.pt_off * 3 * 8, (size_t)d.L * 3 * 8);
    if (r.edge_chi2 && d.in_edges) std::memcpy(r.edge_chi2, h + o_chi + (size_t)d.out_off * 8, (size_t)d.in_edges * 8);
    if (r.edge_depth_pos && d.in_edges) std::memcpy(r.edge_depth_pos, h + o_depth + (size_t)d.out_off, (size_t)d.in_edges);
    r.status = OSH_OK; r.iterations = st.iterations; r.trials = st.trials; r.n_trace = st.n_trace;
    r.chi2_initial = st.chi2_initial;
    for (int k = 0; k < st.n_trace; ++k) { r.chi2_trace[k] = st.chi2_trace[k]; r.lambda_trace[k] = st.lambda_trace[k]; r.trials_trace[k] = st.trials_trace[k]; }
  };
  const int n_threads = default_pack_threads(nw);
  if (n_threads <= 1) {
    for (int w = 0; w < nw; ++w) copy_window(w);
  } else {
    std::atomic<int> next{0};
    auto worker = [&]() { for (int w = next.fetch_add(1); w < nw; w = next.fetch_add(1)) copy_window(w); };
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; ++t) pool.emplace_back(worker);
    worker();
    for (std::thread& t : pool) t.join();
  }
  return OSH_OK;
}

extern "C" int osh_lba_solve(osh_lba_ctx* c, int32_t nw, const osh_lba_problem* pr, osh_lba_result* res) {
  OSH_TRY(osh_lba_upload(c, nw, pr));
  OSH_TRY(osh_lba_optimize(c));
  return osh_lba_download(c, nw, res);
}

// Host view of an int section of arena 0: the host packer's staging, or a copy from the device when the batch was packed there.
static int host_ints(osh_lba_ctx* c, int sec, size_t count, std::vector<int>& store, const int*& out) {
  if (!c->device_packed) { out = c->pb.sec<int>(sec); return OSH_OK; }
  store.resize(std::max<size_t>(count, 1));
  if (count) OSH_HIP(hipMemcpy(store.data(), c->dsec<int>(sec), count * 4, hipMemcpyDeviceToHost));
  out = store.data();
  return OSH_OK;
}

// Debug / parity aid: one linearisation of `window` at the uploaded estimates.
extern "C" int osh_lba_linearize(osh_lba_ctx* c, int32_t window, double* Hpp, double* bp, double* Hll, double* bl,
                                 double* Hpl, double* chi2, double* robust_chi2) {
  if (!c || window < 0 || window >= c->n_windows) { set_error("osh_lba_linearize: bad window"); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const PackedBatch& pb = c->pb;
  OSH_TRY(reset_state(c, nullptr, true));
  OSH_TRY(first_linearisation(c));
  OSH_HIP(hipStreamSynchronize(s));
  const WinDesc& d = pb.win[window];
  std::vector<LmState> h_lm(c->n_windows);
  OSH_HIP(hipMemcpy(h_lm.data(), c->d_lm.p, c->n_windows * sizeof(LmState), hipMemcpyDeviceToHost));
  if (robust_chi2) *robust_chi2 = h_lm[window].chi2_initial;
  if (Hpp && d.P) OSH_HIP(hipMemcpy(Hpp, c->d_Hpp.as<double>() + (size_t)d.fpose_off * 36, (size_t)d.P * 36 * 8, hipMemcpyDeviceToHost));
  if (bp && d.P) OSH_HIP(hipMemcpy(bp, c->d_bp.as<double>() + (size_t)d.fpose_off * 6, (size_t)d.P * 6 * 8, hipMemcpyDeviceToHost));
  std::vector<int> perm_store, eo_store, eo2_store;
  const int* perm = nullptr;   // new -> caller landmark index
  OSH_TRY(host_ints(c, PackedBatch::LMPERM, pb.NL, perm_store, perm));
  perm += d.pt_off;
  if (bl && d.L) {
    std::vector<double> t((size_t)d.L * 3);
    OSH_HIP(hipMemcpy(t.data(), c->d_bl.as<double>() + (size_t)d.pt_off * 3, t.size() * 8, hipMemcpyDeviceToHost));
    for (int j = 0; j < d.L; ++j) std::memcpy(bl + (size_t)perm[j] * 3, &t[(size_t)j * 3], 24);
  }
  if (Hll && d.L) {
    std::vector<double> up((size_t)d.L * 6);
    OSH_HIP(hipMemcpy(up.data(), c->d_Hll.as<double>() + (size_t)d.pt_off * 6, up.size() * 8, hipMemcpyDeviceToHost));
    for (int j = 0; j < d.L; ++j) {
      const double* u = &up[(size_t)j * 6];
      double* o = Hll + (size_t)perm[j] * 9;
      o[0] = u[0]; o[1] = u[1]; o[2] = u[2]; o[3] = u[1]; o[4] = u[3]; o[5] = u[4]; o[6] = u[2]; o[7] = u[4]; o[8] = u[5];
    }
  }
  if (Hpl && d.in_edges) {
    OSH_TRY(c->d_dbg.reserve(std::max<size_t>(pb.NE * 18 * 8, 8)));
    hipLaunchKernelGGL(c->kp_debug_hpl, dim3((unsigned)pb.n_chunks), dim3(kBlock), 0, s, c->bv, c->d_dbg.as<double>());
    OSH_TRY(launch_check("k_debug_hpl"));
    OSH_HIP(hipStreamSynchronize(s));
    std::vector<double> hs((size_t)d.E * 18);
    if (d.E) OSH_HIP(hipMemcpy(hs.data(), c->d_dbg.as<double>() + (size_t)d.edge_off * 18, hs.size() * 8, hipMemcpyDeviceToHost));
    std::memset(Hpl, 0, (size_t)d.in_edges * 18 * 8);
    const int *eo = nullptr, *eo2 = nullptr;
    OSH_TRY(host_ints(c, PackedBatch::EORIG, pb.NE, eo_store, eo));
    eo += d.edge_off;
    if (pb.has_rig) { OSH_TRY(host_ints(c, PackedBatch::EORIG2, pb.NE, eo2_store, eo2)); eo2 += d.edge_off; }
    // the two edges of a merged fisheye-rig pair share one Hessian block: both report it (their sum)
    for (int x = 0; x < d.E; ++x) {
      std::memcpy(Hpl + (size_t)eo[x] * 18, &hs[(size_t)x * 18], 18 * 8);
      if (eo2 && eo2[x] >= 0) std::memcpy(Hpl + (size_t)eo2[x] * 18, &hs[(size_t)x * 18], 18 * 8);
    }
  }
  if (chi2 && d.in_edges) {
    // mark every window evaluated so k_finalize emits chi2 of the current state
    for (auto& st : h_lm) { st.iterations = 1; st.last_eval_sel = st.sel; }
    OSH_HIP(hipMemcpy(c->d_lm.p, h_lm.data(), c->n_windows * sizeof(LmState), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(c->kp_finalize, dim3((unsigned)pb.n_chunks), dim3(kBlock), c->fin_lds, s, c->bv);
    OSH_TRY(launch_check("k_finalize"));
    OSH_HIP(hipStreamSynchronize(s));
    OSH_HIP(hipMemcpy(chi2, c->d_out_chi2.as<double>() + d.out_off, (size_t)d.in_edges * 8, hipMemcpyDeviceToHost));
  }
  c->optimized = false;
  return OSH_OK;
}

// Debug / parity aid: one LM trial of every window at the uploaded estimates with lambda
// forced to `lambda`; exports S (dense, upper valid), the reduced rhs and x = (x_p, x_l).
extern "C" int osh_lba_debug_trial(osh_lba_ctx* c, int32_t window, double lambda, double* S, double* bs, double* x) {
  if (!c || window < 0 || window >= c->n_windows) { set_error("osh_lba_debug_trial: bad window"); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const PackedBatch& pb = c->pb;
  OSH_TRY(reset_state(c, nullptr, true));
  LAUNCH(OSH_K_LINEARIZE, c->kp_lin_lm, pb.n_chunks, kBlock, c->lin_lds, c->bv);
  LAUNCH(OSH_K_LIN_POSE, c->kp_pose_only, pb.n_sym, 64, 0, c->bv, 0, 0);
  LAUNCH(OSH_K_POSE_HESS, k_pose_reduce, (pb.NFP + 1) / 2, 64, 0, c->bv, 0);
  LAUNCH(OSH_K_CONTROL, k_control, c->n_windows, 64, 0, c->bv, 0);
  OSH_HIP(hipStreamSynchronize(s));
  std::vector<LmState> h_lm(c->n_windows);
  OSH_HIP(hipMemcpy(h_lm.data(), c->d_lm.p, c->n_windows * sizeof(LmState), hipMemcpyDeviceToHost));
  for (auto& st : h_lm) { st.lambda = lambda; st.need_dl = 1; }
  OSH_HIP(hipMemcpy(c->d_lm.p, h_lm.data(), c->n_windows * sizeof(LmState), hipMemcpyHostToDevice));
  const WinDesc& d = pb.win[window];
  LAUNCH(OSH_K_LIN_AUX, c->kp_lin_lm, pb.n_chunks, kBlock, c->lin_lds, c->bv);
  LAUNCH(OSH_K_SCHUR, c->kp_schur_sym, pb.n_sym, 64, 0, c->bv, 0, 1);
  LAUNCH(OSH_K_SCHUR_CROSS, c->kp_schur_cross, pb.n_items - pb.n_sym, 64, 0, c->bv, (int)pb.n_sym, 1);
  OSH_TRY(launch_schur_reduce(c));
  OSH_HIP(hipStreamSynchronize(s));
  if (S && d.n) OSH_HIP(hipMemcpy(S, c->d_S.as<double>() + d.S_off, (size_t)d.n * d.n * 8, hipMemcpyDeviceToHost));
  if (bs && d.n) OSH_HIP(hipMemcpy(bs, c->d_bs.as<double>() + (size_t)d.fpose_off * 6, (size_t)d.n * 8, hipMemcpyDeviceToHost));
  OSH_TRY(launch_solve(c, s));
  hipLaunchKernelGGL(c->kp_backsub, dim3((unsigned)pb.n_chunks), dim3(kBlock), c->backsub_lds, s, c->bv);
  OSH_TRY(launch_check("k_backsub"));
  OSH_HIP(hipStreamSynchronize(s));
  if (x) {
    if (d.n) OSH_HIP(hipMemcpy(x, c->d_xp.as<double>() + (size_t)d.fpose_off * 6, (size_t)d.n * 8, hipMemcpyDeviceToHost));
    // x_l = X_trial - X_cur, back in the caller's landmark order
    std::vector<double> a((size_t)d.L * 3), b((size_t)d.L * 3);
    if (d.L) {
      std::vector<int> perm_store;
      const int* perm = nullptr;
      OSH_TRY(host_ints(c, PackedBatch::LMPERM, pb.NL, perm_store, perm));
      perm += d.pt_off;
      OSH_HIP(hipMemcpy(a.data(), c->d_pt[1].as<double>() + (size_t)d.pt_off * 3, a.size() * 8, hipMemcpyDeviceToHost));
      OSH_HIP(hipMemcpy(b.data(), c->d_pt[0].as<double>() + (size_t)d.pt_off * 3, b.size() * 8, hipMemcpyDeviceToHost));
      for (int j = 0; j < d.L; ++j)
        for (int k = 0; k < 3; ++k) x[d.n + (size_t)perm[j] * 3 + k] = a[(size_t)j * 3 + k] - b[(size_t)j * 3 + k];
    }
  }
  c->optimized = false;
  return OSH_OK;
}

// {big, nb, threads, lds_bytes} of the last upload: which factorisation its reduced systems take (solve_plan.h)
extern "C" int osh_lba_get_solver(osh_lba_ctx* c, int32_t out[4]) {
  if (!c || !out || c->n_windows <= 0) { set_error("osh_lba_get_solver: nothing uploaded"); return OSH_ERR_INVALID; }
  out[0] = c->solve_big ? 1 : 0; out[1] = c->solve_nb; out[2] = c->solve_threads; out[3] = (int32_t)c->solve_lds;
  return OSH_OK;
}

// 0: pack uploads on the device (default), 1: on the host (lba_pack.h), -1: default
// rules (OSH_LBA_PACK=host in the environment selects the host packer)
extern "C" int osh_lba_set_pack_mode(osh_lba_ctx* c, int mode) {
  if (!c || mode < -1 || mode > 1) { set_error("osh_lba_set_pack_mode: bad arguments"); return OSH_ERR_INVALID; }
  c->pack_mode = mode;
  return OSH_OK;
}

// Test hook: packs the problems with the device packer AND the host packer and compares every section of the two layouts.
extern "C" int osh_lba_pack_compare(osh_lba_ctx* c, int32_t nw, const osh_lba_problem* pr, int64_t stats[4]) {
  if (!c || nw <= 0 || !pr) { set_error("osh_lba_pack_compare: bad arguments"); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(c->device));
  OSH_HIP(hipStreamSynchronize(c->stream));
  return device_pack_compare(c->dpack, c->stream, nw, pr, stats);
}

extern "C" int osh_lba_set_profiling(osh_lba_ctx* c, int enable) {
  if (!c) return OSH_ERR_INVALID;
  OSH_HIP(hipSetDevice(c->device));
  if (enable) OSH_TRY(c->timer.init());
  c->timer.enabled = enable != 0;
  c->dpack.timing = enable != 0;
  c->timer.reset();
  return OSH_OK;
}

extern "C" int osh_lba_get_profile(osh_lba_ctx* c, int64_t launches[OSH_K_COUNT], double total_ms[OSH_K_COUNT]) {
  if (!c || !launches || !total_ms) return OSH_ERR_INVALID;
  for (int k = 0; k < OSH_K_COUNT; ++k) { launches[k] = c->timer.launches[k]; total_ms[k] = c->timer.total_ms[k]; }
  return OSH_OK;
}

extern "C" int osh_lba_get_plan_stats(osh_lba_ctx* c, int64_t stats[8]) {
  if (!c || !stats || c->n_windows <= 0) { set_error("osh_lba_get_plan_stats: nothing uploaded"); return OSH_ERR_INVALID; }
  stats[0] = (int64_t)c->pb.n_items; stats[1] = (int64_t)c->pb.n_sym; stats[2] = c->pb.tile_steps; stats[3] = c->pb.pair_blocks;
  stats[4] = (int64_t)c->pb.n_contrib; stats[5] = (int64_t)c->pb.n_rblk; stats[6] = (int64_t)c->pb.n_recs; stats[7] = (int64_t)c->pb.n_ccontrib;
  return OSH_OK;
}

// Device-side cost of the last upload packed on the device (HIP events; enable with osh_lba_set_profiling before the upload):
// ms[0] H2D of the staged problem, ms[1..3] k_pack_pre1 / k_pack_pre2 / k_pack_post, ms[4] staged bytes, ms[5] 1 if the batch was packed on the
// device, ms[6..29] shader-clock cycles per phase of the three kernels (mean over the windows)
extern "C" int osh_lba_get_pack_profile(osh_lba_ctx* c, double ms[30]) {
  if (!c || !ms) return OSH_ERR_INVALID;
  for (int k = 0; k < 4; ++k) ms[k] = c->dpack.ev_ms[k];
  ms[4] = (double)c->dpack.raw_bytes; ms[5] = c->device_packed ? 1.0 : 0.0;
  for (int k = 0; k < 24; ++k) ms[6 + k] = c->dpack.cyc_mean[k];
  return OSH_OK;
}

extern "C" int osh_lba_get_upload_times(osh_lba_ctx* c, double ms[2]) {
  if (!c || !ms) return OSH_ERR_INVALID;
  ms[0] = c->upload_pack_ms; ms[1] = c->upload_copy_ms;
  return OSH_OK;
}

extern "C" const char* osh_lba_kernel_name(int k) {
  // pinhole instantiations reading float32 records (<true, ..> for a fisheye batch, <.., false> when a record is not exact in float32)
  // slot OSH_K_RESIDUAL keeps its name and reports no launches: the trial residual has been the tail of k_backsub since round 3
  static const char* names[OSH_K_COUNT] = {"k_lin_lm<false, true>", "k_pose_reduce", "k_schur_fused<true, false> (mode 1)", "k_solve", "k_backsub<false, true>",
                                           "k_residual<false, true>", "k_control", "k_schur_reduce", "k_schur_fused<false, false>",
                                           "k_lin_lm<false, true> (factors only)", "k_schur_fused<true, false, false, true> (pose side alone)"};
  return (k >= 0 && k < OSH_K_COUNT) ? names[k] : "?";
}
