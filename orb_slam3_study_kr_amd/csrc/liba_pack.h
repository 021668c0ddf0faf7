// liba_pack.h -- host-side packing of a batch of inertial BA windows into the flat layout k_liba reads (liba_device.hip).  Pure host
// C++: no HIP call and no device code, so osh_liba_pack_check (liba_pack_check.cpp) runs all of it without a GPU.
//
// The inertial counterpart of lba_pack.h.  What it produces, per window:
//   * the window descriptor (LibaDesc): sizes, offsets into the batch's arrays, camera and rig extrinsics, controller parameters,
//     and for map-sized problems the band of the reduced system;
//   * edges sorted landmark-major, inside a landmark by pose (a fisheye rig's left EdgeMono(0) + right EdgeMono(1) on one
//     (keyframe, landmark) Hessian block stay two edges next to each other, the block being the left one's);
//   * the pose-by-pose walk order of the linearisation (pel_off, pel_edge) and the (landmark, pose) -> block table (lm_pose_edge);
//   * the inertial links with a colour each, so that the links of one colour share no keyframe.
// Everything lands in ONE input arena that the caller supplies (pinned memory in the device path) and copies to the device in one
// transfer; LibaLayout also places the result arena and the work arena that follow it on the device.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"       // Section, Layout
#include "ldlt_block.h"   // ldlt_row_stride, ldlt_lds_doubles

namespace osh {

constexpr int kLT = 256;      // threads of a block: one wavefront per SIMD, so a phase may use all 512 registers (with 512 threads the
                              // per-edge code spilled: 1.2 KB of scratch per lane)
constexpr int kLNB = 24;      // LDL^T panel width (12 or 6 for windows whose 24-wide panels do not fit LDS: k_liba<NB>)
constexpr int kLG = 32;       // blocks per window at most (one XCD's worth of a group)
constexpr int kPoseChunks = 8;   // a pose row's edges are summed in at most this many chunks
constexpr int kLinkQ = 832;   // per link: J^T W J (24x24), -J^T W r (24), then J (9x24), -W r (9), rho'
// LDS scratch: the LDL^T panels of the reduced system when they fit one block's LDS (NB = 24: up to 51 keyframes, every LocalInertialBA /
// MergeInertialBA window, liba_solve); beyond that the group factorises in global memory (NB = 6 names that variant, liba_solve_group)
// and LDS holds its 16 x 16 blocks and two vectors only.  600 keyframes = a dense 9000 x 9000 system (H and S: 1.3 GB).
constexpr int kLibaMaxKeyframes = 1200;
constexpr size_t kLibaLdsBytes = 160 * 1024 - 64;
__host__ __device__ constexpr size_t liba_scratch_doubles(int NB, int W) {
  const size_t need = NB == kLNB ? ldlt_lds_doubles(NB, W, kLT) : (size_t)(6 * 256 + 64 + W + 32);
  return need > 512 ? need : 512;
}

struct LibaDesc {
  int N, NV, K, L, E, NL, n, max_iter;
  int pose_off, vel_off, pt_off, edge_off, link_off, lmoff_off, pel_off, peloff_off, lmpose_off;
  long long H_off;       // n*n doubles (H and S use the same offset in their own arrays)
  int b_off;             // n doubles
  double Rcb[9], tcb[3], tbc[3], cam[5];
  double kb8[4];   // KannalaBrandt8 k1..k4 (osh_liba_problem.kb8)
  int kb8_on;      // 1: mono edges project through KannalaBrandt8
  int rig_on;      // 1: fisheye stereo rig, OSH_EDGE_RIGHT edges are EdgeMono(1) on camera 1 of ImuCamPose (src/G2oTypes.cc:56-66)
  double Rrl[9], trl[3], Rcb1[9], tbc1[3], cam2[8];   // Trl; Rcb[1] = Rrl Rcb[0]; tbc[1] = -Rbc[1] tcb[1]; right camera fx fy cx cy k1..k4
  double huber_mono, huber_stereo, huber_inertial, lambda_init;
  int n_colours;         // inertial links are coloured so that the links of one colour share no keyframe (liba_pack_window)
  int il;                // layout of the reduced unknowns: 0 = [pose 6] x N then [velocity, gyro bias, accelerometer bias 9] x N (every
                         // LocalInertialBA window), 1 = [pose 6 | v bg ba 9] per keyframe (map-sized problems: with the keyframes in
                         // temporal order the reduced system is then BANDED -- landmarks and IMU links couple nearby keyframes only)
  int bw, bw_kf;         // il = 1: entries (r, c) with |r - c| > bw are structurally zero and never touched; bw_kf = the same in keyframes
};

struct LibaOut {
  double chi2_initial, chi2_final;
  int iterations, trials, n_trace, sel;
  int chunks;          // C, the chunks per pose row (written by a run that stops after a stage only)
  double chi2_trace[OSH_LBA_MAX_TRACE], lambda_trace[OSH_LBA_MAX_TRACE];
  int trials_trace[OSH_LBA_MAX_TRACE];
  long long prof[8];   // shader-clock cycles of block 0 per phase: linearise, assembly, Dinv, Schur, LDL^T, back-substitution, errors, outputs
};

// sums over the windows of a batch: keyframes, keyframes with an IMU state, landmarks, edges, links, entries of H, of b, of lm_off, of
// pel_off, edges of optimisable poses, entries of lm_pose_edge; the largest reduced system
struct LibaTotals {
  size_t K = 0, NV = 0, L = 0, E = 0, NL = 0, Htot = 0, btot = 0, LO = 0, PO = 0, EF = 0, LP = 0;
  int n_max = 0;
};

// what the describe / band / pack steps fill; err and msg as in PackedBatch of lba_pack.h (the caller passes msg on to set_error)
struct LibaPack {
  std::vector<LibaDesc> desc;
  LibaTotals tot;
  int err = OSH_OK;
  char msg[400] = {0};
  __attribute__((format(printf, 3, 4))) int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    return err = code;
  }
};

// the environment knobs of a call.  Read once at the top of every call and never cached: the tests change them between calls.
struct LibaKnobs {
  bool dense;           // OSH_LIBA_DENSE: map-sized problems keep the dense layout
  int group;            // OSH_LIBA_GROUP: blocks per window (1, 2, 4, 8, 16 or 32; 0: not set)
  bool heavy_barrier;   // OSH_LIBA_HEAVY_BARRIER: LibaView::force_heavy
  bool test_abort;      // OSH_LIBA_TEST_ABORT: LibaView::test_abort on the first launch of a group
};
inline LibaKnobs liba_read_knobs() {
  LibaKnobs k{std::getenv("OSH_LIBA_DENSE") != nullptr, 0, std::getenv("OSH_LIBA_HEAVY_BARRIER") != nullptr, std::getenv("OSH_LIBA_TEST_ABORT") != nullptr};
  if (const char* gs = std::getenv("OSH_LIBA_GROUP")) { const int gv = std::atoi(gs); if (gv == 1 || gv == 2 || gv == 4 || gv == 8 || gv == 16 || gv == 32) k.group = gv; }
  return k;
}

struct LibaScratch { std::vector<int> cnt, fill, order, place, lo, hi; };

// Validates sizes, indices, kinds and the link / bias rules of every window and fills the descriptors (all but n_colours, which the
// packing finds, and the band) and the totals.  max_iter >= 0 / lambda_init >= 0 replace the problems' own (the debug exports).
inline int liba_describe(int nw, const osh_liba_problem* pr, int max_iter, double lambda_init, LibaPack& pk) {
  pk.desc.assign(nw, LibaDesc{});
  LibaTotals& t = pk.tot = LibaTotals();
  for (int w = 0; w < nw; ++w) {
    const osh_liba_problem& p = pr[w];
    if (p.n_opt <= 0 || p.n_fixed_imu < 0 || p.n_fixed_imu > 1 || p.n_fixed < 0 || p.n_points < 0 || p.n_edges < 0 || p.n_links < 0 ||
        p.max_iterations > OSH_LBA_MAX_TRACE) return pk.fail(OSH_ERR_INVALID, "window %d: bad sizes", w);
    LibaDesc& d = pk.desc[w];
    d.N = p.n_opt; d.NV = p.n_opt + p.n_fixed_imu; d.K = d.NV + p.n_fixed; d.L = p.n_points; d.E = p.n_edges; d.NL = p.n_links;
    d.n = 15 * d.N; d.max_iter = max_iter >= 0 ? max_iter : p.max_iterations; d.n_colours = 0; d.il = 0; d.bw = d.n; d.bw_kf = d.N;
    d.pose_off = (int)t.K; d.vel_off = (int)t.NV; d.pt_off = (int)t.L; d.edge_off = (int)t.E; d.link_off = (int)t.NL; d.lmoff_off = (int)t.LO;
    d.peloff_off = (int)t.PO; d.pel_off = (int)t.EF; d.lmpose_off = (int)t.LP; d.H_off = (long long)t.Htot; d.b_off = (int)t.btot;
    std::memcpy(d.Rcb, p.Rcb, 72); std::memcpy(d.tcb, p.tcb, 24); std::memcpy(d.tbc, p.tbc, 24); std::memcpy(d.cam, p.cam, 40);
    d.huber_mono = p.huber_mono; d.huber_stereo = p.huber_stereo; d.huber_inertial = p.huber_inertial;
    d.lambda_init = lambda_init >= 0 ? lambda_init : p.lambda_init;
    d.kb8_on = p.kb8 ? 1 : 0;
    for (int k = 0; k < 4; ++k) d.kb8[k] = p.kb8 ? p.kb8[k] : 0.0;
    d.rig_on = (p.kb8 && p.cam2 && p.trl) ? 1 : 0;
    if (d.rig_on) {
      // ImuCamPose(KeyFrame*) camera 1 (src/G2oTypes.cc:56-66): Rcb[1] = Rrl Rcb[0], tcb[1] = Rrl tcb[0] + trl, tbc[1] = -Rbc[1] tcb[1]
      double tcb1[3];
      for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) d.Rrl[i * 3 + j] = p.trl[i * 4 + j]; d.trl[i] = p.trl[i * 4 + 3]; }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double a = 0.0;
          for (int k = 0; k < 3; ++k) a += d.Rrl[i * 3 + k] * d.Rcb[k * 3 + j];
          d.Rcb1[i * 3 + j] = a;
        }
      for (int i = 0; i < 3; ++i) tcb1[i] = d.Rrl[i * 3] * d.tcb[0] + d.Rrl[i * 3 + 1] * d.tcb[1] + d.Rrl[i * 3 + 2] * d.tcb[2] + d.trl[i];
      for (int i = 0; i < 3; ++i) d.tbc1[i] = -(d.Rcb1[i] * tcb1[0] + d.Rcb1[3 + i] * tcb1[1] + d.Rcb1[6 + i] * tcb1[2]);
      std::memcpy(d.cam2, p.cam2, 64);
    }
    if (p.kb8)
      for (int e = 0; e < p.n_edges; ++e)
        if (p.edge_kind[e] == OSH_EDGE_STEREO) return pk.fail(OSH_ERR_UNSUPPORTED, "window %d: a KannalaBrandt8 window takes monocular edges only (edge %d)", w, e);
    size_t ef = 0;
    for (int e = 0; e < p.n_edges; ++e) {
      if (p.edge_pose[e] < 0 || p.edge_pose[e] >= d.K || p.edge_point[e] < 0 || p.edge_point[e] >= d.L || p.edge_kind[e] > OSH_EDGE_RIGHT)
        return pk.fail(OSH_ERR_INVALID, "window %d edge %d: index or kind out of range", w, e);
      if (p.edge_kind[e] == OSH_EDGE_RIGHT && !d.rig_on) return pk.fail(OSH_ERR_INVALID, "window %d edge %d: a right-camera edge (EdgeMono(1)) needs kb8, cam2 and trl", w, e);
      if (p.edge_pose[e] < d.N) ++ef;
    }
    for (int l = 0; l < p.n_links; ++l)
      if (p.link_prev[l] < 0 || p.link_prev[l] >= d.NV || p.link_cur[l] < 0 || p.link_cur[l] >= d.N)
        return pk.fail(OSH_ERR_INVALID, "window %d link %d: keyframe index out of range", w, l);
    if (p.link_bias)
      for (int l = 0; l < p.n_links; ++l) {
        if (p.link_bias[l] < 0 || p.link_bias[l] >= d.NV) return pk.fail(OSH_ERR_INVALID, "window %d link %d: bias keyframe out of range", w, l);
        if (p.link_bias[l] == p.link_prev[l]) continue;
        // the random-walk terms of the later keyframe are added beside the edge's own terms, by other threads of the same phase
        if (p.link_bias[l] == p.link_cur[l]) return pk.fail(OSH_ERR_UNSUPPORTED, "window %d link %d: the bias vertices of a link cannot be those of its later keyframe", w, l);
        // the random-walk terms of a link's earlier keyframe are summed into the blocks of the edge's own bias vertices
        for (int k = 0; k < 9; ++k)
          if (p.link_info_g[(size_t)l * 9 + k] != 0.0 || p.link_info_a[(size_t)l * 9 + k] != 0.0)
            return pk.fail(OSH_ERR_UNSUPPORTED, "window %d link %d: a link whose bias vertices belong to another keyframe carries no random-walk edges", w, l);
      }
    t.K += d.K; t.NV += d.NV; t.L += d.L; t.E += d.E; t.NL += d.NL; t.Htot += (size_t)d.n * d.n; t.btot += d.n; t.LO += (size_t)d.L + 1;
    t.PO += (size_t)d.N + 1; t.EF += ef; t.LP += (size_t)d.L * d.N;
    t.n_max = std::max(t.n_max, d.n);
  }
  return OSH_OK;
}

// How the reduced system of the largest window is factorised: 24-wide panels in the LDS of one block while they fit (51 keyframes);
// beyond, the whole group factorises in global memory (liba_solve_group; k_liba<6> -- its LDS need, vectors of n doubles, stays below
// what 6-wide panels would take).  W: row stride of the panels, lds: dynamic LDS bytes of the launch.
struct LibaPanels { int NB, W; size_t lds; };
inline int liba_panels(LibaPack& pk, LibaPanels& pan) {
  const int n_max = pk.tot.n_max;
  pan.W = ldlt_row_stride(n_max);
  pan.NB = kLNB;
  if ((liba_scratch_doubles(pan.NB, pan.W) + kLT / 64 + 8) * sizeof(double) > kLibaLdsBytes) pan.NB = 6;
  pan.lds = (liba_scratch_doubles(pan.NB, pan.W) + kLT / 64 + 8) * sizeof(double);
  if (pan.lds > kLibaLdsBytes || n_max > 15 * kLibaMaxKeyframes)
    return pk.fail(OSH_ERR_UNSUPPORTED, "inertial window with %d optimisable keyframes: the device path handles up to %d (LocalInertialBA uses 10 or 25)", n_max / 15, kLibaMaxKeyframes);
  return OSH_OK;
}

// Map-sized problems (the group factorisation in global memory): with the keyframes in temporal order a landmark is seen by nearby
// keyframes and an IMU link joins neighbours, so with the unknowns interleaved per keyframe the reduced system is banded.  The band is
// the largest keyframe distance any landmark or link spans; a loop closure or the one-bias-pair mode of FullInertialBA (every link on
// one keyframe's bias vertices) makes it the whole map, and the problem stays in the dense layout.
inline void liba_band(int nw, const osh_liba_problem* pr, LibaPack& pk, LibaScratch& sc) {
  std::vector<int>&lo = sc.lo, &hi = sc.hi;
  for (int w = 0; w < nw; ++w) {
    const osh_liba_problem& p = pr[w];
    LibaDesc& d = pk.desc[w];
    if (d.N < 32) continue;
    int span = 1;
    lo.assign(d.L, d.N); hi.assign(d.L, -1);
    for (int e = 0; e < p.n_edges; ++e) {
      const int ip = p.edge_pose[e], j = p.edge_point[e];
      if (ip >= d.N) continue;
      lo[j] = std::min(lo[j], ip); hi[j] = std::max(hi[j], ip);
    }
    for (int j = 0; j < d.L; ++j) if (hi[j] >= 0) span = std::max(span, hi[j] - lo[j]);
    for (int l = 0; l < p.n_links; ++l) {
      const int a = p.link_prev[l], c2 = p.link_cur[l], ab = p.link_bias ? p.link_bias[l] : a;
      int mn = c2, mx = c2;
      if (a < d.N) { mn = std::min(mn, a); mx = std::max(mx, a); }
      if (ab < d.N) { mn = std::min(mn, ab); mx = std::max(mx, ab); }
      span = std::max(span, mx - mn);
    }
    if (15 * (span + 1) <= d.n / 2) { d.il = 1; d.bw_kf = span; d.bw = 15 * (span + 1) - 1; }
  }
}

// The sections of the three arenas.  in: every input array, staged in ONE pinned buffer and uploaded in ONE copy.  out: what comes
// back in one copy (LibaOut per window, abort word, final poses / velocities+biases / points, edge chi2 and depth flags).  work: the
// buffers that never leave the device.  Members are named after the LibaView fields they are bound to.
struct LibaLayout {
  Layout in, out, work;
  bool debug = false;   // a debug run keeps the buffers it reports (`kept` below) in `out`, so that they come back with the one download
  // ---- in
  Section<LibaDesc> desc;
  Section<double> pose, vba, pts, e_obs, e_info;
  Section<int> e_pose, e_point, e_orig, lm_off, pel_off, pel_edge, lm_pose_edge, link_prev, link_cur;
  Section<unsigned char> e_kind, link_robust;
  Section<float> link_preint;
  Section<double> link_info, link_info_g, link_info_a;
  Section<unsigned> bar;
  Section<int> abort_flag, link_colour, link_bias;
  // ---- out
  Section<LibaOut> res;
  Section<int> res_abort;
  Section<double> res_pose, res_vba, res_pts, out_chi2;
  Section<unsigned char> out_depth;
  // ---- work
  Section<double> pose1, vba1, eh, ep, bfull, BD, dinv, red;
  // ---- kept: work, or out in a debug run
  Section<double> pts1, Hpl, Hll, bl, H, S, b, bs, x, linkQ, ppart, ctrl;
  // every section in the order taken, for the self check: arena (0 in, 1 out, 2 work), offset, bytes asked for
  struct Extent { int arena; size_t off, bytes; };
  Extent ext[64];
  int n_ext = 0;
  template <class T>
  void take(Layout& a, Section<T>& s, size_t count) {
    s = a.take<T>(count);
    if (n_ext < 64) ext[n_ext++] = Extent{&a == &in ? 0 : (&a == &out ? 1 : 2), s.off, count * sizeof(T)};
  }
};

// The arena offsets are part of the behaviour (they decide what shares a cache line and a page): the order and the types of the take
// calls stay as they are.
inline void liba_layout(int nw, const LibaTotals& t, bool debug, LibaLayout& y) {
  y = LibaLayout();
  y.debug = debug;
  Layout &in = y.in, &out = y.out, &work = y.work, &kept = debug ? y.out : y.work;
  const size_t NK = t.btot / 15;   // optimisable keyframes
  y.take(in, y.desc, nw);
  y.take(in, y.pose, t.K * 24); y.take(in, y.vba, t.NV * 9); y.take(in, y.pts, t.L * 3); y.take(in, y.e_obs, t.E * 3); y.take(in, y.e_info, t.E);
  y.take(in, y.e_pose, t.E); y.take(in, y.e_point, t.E); y.take(in, y.e_orig, t.E); y.take(in, y.lm_off, t.LO); y.take(in, y.pel_off, t.PO);
  y.take(in, y.pel_edge, t.E); y.take(in, y.lm_pose_edge, t.LP); y.take(in, y.link_prev, t.NL); y.take(in, y.link_cur, t.NL);
  y.take(in, y.e_kind, t.E); y.take(in, y.link_robust, t.NL);
  y.take(in, y.link_preint, t.NL * OSH_PREINT_FLOATS);
  y.take(in, y.link_info, t.NL * 81); y.take(in, y.link_info_g, t.NL * 9); y.take(in, y.link_info_a, t.NL * 9);
  y.take(in, y.bar, nw);
  y.take(in, y.abort_flag, 1); y.take(in, y.link_colour, t.NL); y.take(in, y.link_bias, t.NL);
  y.take(out, y.res, nw);
  y.take(out, y.res_abort, 1);
  y.take(out, y.res_pose, NK * 24); y.take(out, y.res_vba, NK * 9); y.take(out, y.res_pts, t.L * 3); y.take(out, y.out_chi2, t.E);
  y.take(out, y.out_depth, t.E);
  y.take(work, y.pose1, t.K * 24); y.take(work, y.vba1, t.NV * 9); y.take(kept, y.pts1, t.L * 3); y.take(work, y.eh, t.E * 9);
  y.take(work, y.ep, t.EF * 27); y.take(work, y.bfull, t.btot); y.take(kept, y.Hpl, t.EF * 18); y.take(work, y.BD, t.EF * 18);
  y.take(kept, y.Hll, t.L * 6); y.take(kept, y.bl, t.L * 3); y.take(work, y.dinv, t.L * 9); y.take(kept, y.H, t.Htot);
  y.take(kept, y.S, t.Htot); y.take(kept, y.b, t.btot); y.take(kept, y.bs, t.btot); y.take(kept, y.x, t.btot);
  y.take(kept, y.linkQ, t.NL * kLinkQ); y.take(kept, y.ppart, NK * kPoseChunks * 27);
  y.take(work, y.red, (size_t)nw * 4 * kLG * 2); y.take(kept, y.ctrl, (size_t)nw * 4);
}

// The links of a window into the input arena, each with the keyframe that stores its bias vertices (default: the earlier one) and a
// colour; d.n_colours = the colours used.
inline void liba_pack_links(const osh_liba_problem& p, LibaDesc& d, const LibaLayout& y, char* base) {
  int *h_lp = y.link_prev.in(base) + d.link_off, *h_lc = y.link_cur.in(base) + d.link_off, *h_lb = y.link_bias.in(base) + d.link_off;
  int* h_col = y.link_colour.in(base) + d.link_off;
  for (int l = 0; l < d.NL; ++l) {
    const size_t g = (size_t)d.link_off + l;
    h_lp[l] = p.link_prev[l]; h_lc[l] = p.link_cur[l]; y.link_robust.in(base)[g] = p.link_robust[l];
    h_lb[l] = p.link_bias ? p.link_bias[l] : p.link_prev[l];
    std::memcpy(y.link_preint.in(base) + g * OSH_PREINT_FLOATS, p.link_preint + (size_t)l * OSH_PREINT_FLOATS, OSH_PREINT_FLOATS * 4);
    std::memcpy(y.link_info.in(base) + g * 81, p.link_info + (size_t)l * 81, 81 * 8);
    std::memcpy(y.link_info_g.in(base) + g * 9, p.link_info_g + (size_t)l * 9, 72); std::memcpy(y.link_info_a.in(base) + g * 9, p.link_info_a + (size_t)l * 9, 72);
    // greedy colouring: the first colour none of the earlier links sharing a keyframe with this one has (a chain takes two)
    int col = 0;
    for (bool clash = true; clash; ) {
      clash = false;
      for (int l2 = 0; l2 < l && !clash; ++l2) {
        if (h_col[l2] != col) continue;
        const int k1[3] = {h_lp[l], h_lc[l], h_lb[l]}, k2[3] = {h_lp[l2], h_lc[l2], h_lb[l2]};
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) clash = clash || k1[a] == k2[b];
      }
      if (clash) ++col;
    }
    h_col[l] = col;
    d.n_colours = std::max(d.n_colours, col + 1);
  }
}

// Window w into the input arena at `base`: the state, the edges landmark-major (counting sort by landmark, then a stable sort by pose
// and kind inside a landmark), lm_off, the pose-by-pose walk order, the (landmark, pose) -> block table, then the links.
// lm_pose_edge must hold -1 everywhere on entry (liba_pack).
inline int liba_pack_window(int w, const osh_liba_problem& p, LibaPack& pk, const LibaLayout& y, char* base, LibaScratch& sc) {
  LibaDesc& d = pk.desc[w];
  double *h_pose = y.pose.in(base), *h_vba = y.vba.in(base), *h_obs = y.e_obs.in(base), *h_info = y.e_info.in(base);
  int *h_ep = y.e_pose.in(base) + d.edge_off, *h_el = y.e_point.in(base) + d.edge_off, *h_eo = y.e_orig.in(base) + d.edge_off;
  int *h_lmo = y.lm_off.in(base) + d.lmoff_off, *po = y.pel_off.in(base) + d.peloff_off, *h_pel = y.pel_edge.in(base) + d.edge_off;
  int* h_lmpe = y.lm_pose_edge.in(base) + d.lmpose_off;
  unsigned char* h_kind = y.e_kind.in(base) + d.edge_off;
  std::vector<int>&cnt = sc.cnt, &fill = sc.fill, &order = sc.order, &place = sc.place;
  for (int k = 0; k < d.K; ++k) {
    double* o = &h_pose[((size_t)d.pose_off + k) * 24];
    std::memcpy(o, p.pose_Rcw + 9 * k, 72); std::memcpy(o + 9, p.pose_tcw + 3 * k, 24);
    std::memcpy(o + 12, p.pose_Rwb + 9 * k, 72); std::memcpy(o + 21, p.pose_twb + 3 * k, 24);
  }
  for (int k = 0; k < d.NV; ++k) {
    double* o = &h_vba[((size_t)d.vel_off + k) * 9];
    std::memcpy(o, p.vel + 3 * k, 24); std::memcpy(o + 3, p.bias_g + 3 * k, 24); std::memcpy(o + 6, p.bias_a + 3 * k, 24);
  }
  if (d.L) std::memcpy(y.pts.in(base) + (size_t)d.pt_off * 3, p.points, (size_t)d.L * 24);
  cnt.assign((size_t)d.L + 1, 0);
  for (int e = 0; e < d.E; ++e) cnt[p.edge_point[e] + 1]++;
  for (int j = 0; j < d.L; ++j) cnt[j + 1] += cnt[j];
  fill.assign(cnt.begin(), cnt.end() - 1);
  order.resize(d.E);
  for (int e = 0; e < d.E; ++e) order[fill[p.edge_point[e]]++] = e;
  for (int j = 0; j <= d.L; ++j) h_lmo[j] = cnt[j];
  for (int j = 0; j < d.L; ++j) {
    std::stable_sort(order.begin() + cnt[j], order.begin() + cnt[j + 1], [&](int a, int b) {
      return p.edge_pose[a] != p.edge_pose[b] ? p.edge_pose[a] < p.edge_pose[b] : p.edge_kind[a] < p.edge_kind[b];
    });
    for (int x = cnt[j]; x < cnt[j + 1]; ++x) {
      if (x > cnt[j] && p.edge_pose[order[x]] == p.edge_pose[order[x - 1]]) {
        // one Hessian block, two edges: only the left EdgeMono(0) + right EdgeMono(1) of a fisheye rig (src/Optimizer.cc:2737-2835)
        const bool pair = p.edge_kind[order[x]] == OSH_EDGE_RIGHT && p.edge_kind[order[x - 1]] == OSH_EDGE_MONO &&
                          !(x - 1 > cnt[j] && p.edge_pose[order[x - 2]] == p.edge_pose[order[x]]);
        if (!pair)
          return pk.fail(OSH_ERR_UNSUPPORTED, "window %d: landmark %d is observed twice by keyframe %d with edge kinds that do not form a left + right pair", w, j, p.edge_pose[order[x]]);
        continue;   // the pair's block is the first edge's
      }
      if (p.edge_pose[order[x]] < d.N) h_lmpe[(size_t)j * d.N + p.edge_pose[order[x]]] = x;
    }
  }
  for (int i = 0; i <= d.N; ++i) po[i] = 0;
  for (int x = 0; x < d.E; ++x) {
    const int e = order[x];
    h_ep[x] = p.edge_pose[e]; h_el[x] = p.edge_point[e]; h_kind[x] = p.edge_kind[e]; h_eo[x] = e; h_info[(size_t)d.edge_off + x] = p.edge_info[e];
    for (int k = 0; k < 3; ++k) h_obs[((size_t)d.edge_off + x) * 3 + k] = p.edge_obs[3 * e + k];
    if (p.edge_pose[e] < d.N) po[p.edge_pose[e] + 1]++;
  }
  for (int i = 0; i < d.N; ++i) po[i + 1] += po[i];
  fill.assign(po, po + d.N);
  int nfix = po[d.N];   // the fixed keyframes' edges follow the optimisable ones in the walk order of the linearisation
  place.assign((size_t)d.E, -1);   // place of each optimisable-pose edge in that order
  for (int x = 0; x < d.E; ++x) {
    const int ip = h_ep[x];
    if (ip < d.N) place[x] = fill[ip];
    h_pel[ip < d.N ? fill[ip]++ : nfix++] = x;
  }
  // (landmark, pose) -> place of the pair's block: Hpl and B Dinv are stored pose by pose, a landmark's neighbours next to it
  for (size_t k = 0; k < (size_t)d.L * d.N; ++k) { int& x = h_lmpe[k]; if (x >= 0) x = place[x]; }
  liba_pack_links(p, d, y, base);
  return OSH_OK;
}

// Every window of the batch into the input arena at `base` (y.in.bytes of it), then the descriptors.
inline int liba_pack(int nw, const osh_liba_problem* pr, LibaPack& pk, const LibaLayout& y, char* base, LibaScratch& sc) {
  std::memset(y.lm_pose_edge.in(base), 0xff, pk.tot.LP * 4);
  std::memset(y.bar.in(base), 0, nw * sizeof(unsigned));
  std::memset(y.abort_flag.in(base), 0, sizeof(int));
  for (int w = 0; w < nw; ++w)
    if (liba_pack_window(w, pr[w], pk, y, base, sc) != OSH_OK) return pk.err;
  std::memcpy(y.desc.in(base), pk.desc.data(), nw * sizeof(LibaDesc));
  return OSH_OK;
}

}  // namespace osh
