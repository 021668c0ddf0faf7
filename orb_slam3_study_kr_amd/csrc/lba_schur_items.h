// lba_schur_items.h -- k_schur_fused, one wavefront per item of schur_plan.h.  DESIGN.md sections 4 and 25.
#pragma once
#include <type_traits>
#include "lba_chunk.h"

namespace osh {
// --------------------------------------------------------------------------------------------
// k_schur_fused: the pose side of the linearisation and the landmark products of the Schur complement
// (block_solver.hpp:381-432), one wavefront per ITEM of schur_plan.h (landmarks that share their set of optimisable
// observers).  Per chunk of 8 landmarks lane (l, s) owns the edge of landmark l / row pose X[s]:
//   edge description (Xc, Q, g) at the current estimates from the 32-byte observation record, the landmark and the
//   lane's pose (kept in LDS)                                           -> nothing 6x3 is read from memory
//   pose side (once per iteration): Hpp_s += D^T Q D, b_p(s) += D^T g in registers, one 27-double contribution
//   per (item, pose) at the end, reduced in plan order by k_pose_reduce          (base_binary_edge.hpp:55-120)
//   Schur side (every trial): the rows of  W F,  W = Hpl block = D^T Q R,  F F^T = (Hll + lambda I)^-1 from k_lin_lm,
//   stored as a [row][k] image in LDS (row = 6 s + r, k = 3 l + m; row stride 25 doubles: conflict-free MFMA reads),
//   and the rhs term (W F)(F^T b_l) (the _coefficients term, block_solver.hpp:404-409).
// S_ab -= (W_a F)(W_b F)^T is then 6 k-steps of v_mfma_f64_16x16x4_f64 per 16x16 tile, BOTH operands read from the one
// image for symmetric items; the accumulators stay in registers across the chunks of the item.  At the end every live
// pose pair (sa, sb) is written as one 6x6 contribution; k_schur_reduce sums them in plan order.
//   SYM: X == Y, only the tiles on and above the diagonal; owns the pose side and the rhs term.
//   cross items (parts a < b of a landmark with more than 8 optimisable observers): a second image for the Y poses; with at most
//   4 of them (pinhole) that image is filled for two chunks at a time by one 16 x 4 pass (cross_pairs).
//   mode 0: pose side only (the first round of optimize(): computeLambdaInit needs Hpp before any Schur product)
//   mode 1: Schur products, and the pose side when this round opened an iteration other than the first
//   POSE_ONLY (symmetric items, launched with mode 0): the instantiation of the first round of optimize().  Nothing of the Schur
//   side exists in it -- no accumulator tiles, no landmark factors, no image, no multiply, no contribution store -- so it runs in
//   half the registers of the full kernel called with mode 0 (124 against 254).  The lane's edge description, core_pose_side, the
//   chunk walk, the lane reduction and the hcontrib store are the statements of the full kernel: Hpp, b_p and lambda_0 are the same bits
//   (tests/test_gpu_lba_pose_only.py; OSH_LBA_POSE_PASS_FULL at upload keeps the full kernel for this launch).
// --------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kSiLm = 8;               // landmarks per chunk, items of 6 .. 8 row poses (and every cross item)
constexpr int kSiRows = 6 * kItemPoses;
// Lane mappings of a chunk, LM landmarks x PS pose lanes (lane = l * PS + s): 8 x 8, and for symmetric items of at most 5 / at most 4
// row poses 12 x 5 / 16 x 4 -- on the headline window 26 % / 24 % of the symmetric chunks belong to such items and left 3 / 4..7 of their
// 8 pose lanes empty.  The image is [6 PS rows, padded to whole 16-row tiles][3 LM + 1]: 48 x 25, 32 x 37, 32 x 49 doubles.  The k
// steps run over the same sequence of (landmark, component) columns whatever the chunk size (24, 36 and 48 are multiples of 4), so
// the Schur products are the same bits as with 8 x 8 chunks.  (32 x 2 for items of one or two poses -- 18 % of the chunks -- was
// measured too and gained nothing over 16 x 4: with one tile the 24 k steps of such a chunk are one dependent MFMA chain.)
constexpr int kSiImage = 32 * 49;
// BLK (symmetric pinhole items, unless OSH_LBA_SCHUR_TILES is set at upload): the tiles of which only a part is ever stored are formed
// from 4 x 4 blocks, four to a v_mfma_f64_4x4x4_4b_f64 (17 cycles against the 64 of a 16x16x4, the same bits entry by entry and
// (r, c) == (c, r): profiles/ubench/mfma_f64_blocks.hip).  Of block q = (lane >> 2) & 3 a lane holds A[row = lane & 3][k = lane >> 4],
// B[col = lane & 3][k = lane >> 4] and D[row = lane >> 4][col = lane & 3], so the tile operand a[t] (image row 16 t + (lane & 15)) is
// block row q of tile t for the four blocks at once, on either side.  With nx row poses the image has 6 nx rows:
//   a diagonal tile of four live block rows: a[t] x a[t] (blocks (q, q)), a[t] x a[t] turned by one block row ((q, q + 1 mod 4): (3, 0)
//     is (0, 3) mirrored) and by two ((0, 2), (1, 3); the other two repeat them): 3 instructions, 51 cycles instead of 64
//   the last tile column when only L < 4 of its block rows hold image rows (nx = 1 .. 4, 6, 7): a[ti] x block row c of it, the same
//     for all four blocks, c < L, for every tile row ti up to the diagonal: L instructions, and on the diagonal blocks (q <= c) only
//   every other tile: 16x16x4 as before.
// Every instruction of k step ks reads image columns 4 ks .. 4 ks + 3: the k sequence of every entry is the one of the tiles.
// (schur_plan.h: schur_live_blocks, and schur_step for the instruction counts.)

constexpr int kSiPoseRed = 14 * 64;    // the lane reduction of the pose side: 14 of the 27 entries of every lane at a time

template <bool SYM, bool KB8, bool BLK = false, bool POSE_ONLY = false>
__global__ __launch_bounds__(64, KB8 ? 1 : 2) void k_schur_fused(BatchView bv, int item_base, int mode) {
  static_assert(!BLK || (SYM && !KB8), "block path: symmetric pinhole items");
  static_assert(!POSE_ONLY || (SYM && !BLK), "pose side alone: symmetric items, no products");
  constexpr bool kSchur = !POSE_ONLY;
  // (the wider mappings: symmetric pinhole items only; POSE_ONLY: no image, the scratch of the lane reduction alone)
  constexpr int kImage = POSE_ONLY ? kSiPoseRed : ((SYM && !KB8) ? kSiImage : kSiRows * (3 * kSiLm + 1));
  static_assert(kImage >= kSiPoseRed, "the lane reduction of the pose side goes through the image buffer");
  __shared__ double shA[kImage];
  __shared__ double shB[SYM ? 1 : kSiRows * (3 * kSiLm + 1)];
  __shared__ double shPose[(SYM ? 1 : 2) * 8 * kPoseRec];
  __shared__ int shP[64 + 8];
  const int item_idx = item_base + blockIdx.x;
  const SItem it = bv.sitems[item_idx];
  const WinDesc wd = bv.win[it.win];   // by value: the fields stay in SGPRs across the kernel's stores
  const LmView st = lm_view(bv.lm, it.win);
  if (!st.active) return;
  const bool do_hpp = SYM && (mode == 0 ? st.need_lin != 0 : (st.lin_now != 0 && st.iter > 0));
  const bool do_schur = kSchur && mode != 0;
  if (!do_hpp && !do_schur) return;
  const int lane = threadIdx.x;
  const int nx = it.shape & 0xff, ny = (it.shape >> 8) & 0xff;
  const int TX = (6 * nx + 15) >> 4, TY = (6 * ny + 15) >> 4;
  if (kSchur) shP[lane] = bv.spair[(size_t)item_idx * 64 + lane];
  if (lane < 8) shP[64 + lane] = bv.scslot[(size_t)item_idx * 8 + lane];
  {
    // poses of the item's slots -> LDS (lanes 0..7: row poses, lanes 8..15: column poses of a cross item)
    const double* poses = bv.pose_state[st.sel] + (size_t)wd.pose_off * 7;
    const double* cams = bv.pose_cam + (size_t)wd.pose_off * 5;
    const int side = lane >> 3, s8 = lane & 7;
    if (side < (SYM ? 1 : 2)) {
      const int ip = side == 0 ? bv.sposex[(size_t)item_idx * 8 + s8] : bv.sposey[(size_t)item_idx * 8 + s8];
      double qt[7], cam[5], Rm[9];
#pragma unroll
      for (int k = 0; k < 7; ++k) qt[k] = ip >= 0 ? poses[(size_t)ip * 7 + k] : 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) cam[k] = ip >= 0 ? cams[(size_t)ip * 5 + k] : 0.0;
      dev::quat_to_R(qt, Rm);
      double* dst = shPose + (side * 8 + s8) * kPoseRec;
#pragma unroll
      for (int k = 0; k < 7; ++k) dst[k] = qt[k];
#pragma unroll
      for (int k = 0; k < 5; ++k) dst[7 + k] = cam[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) dst[12 + k] = Rm[k];
    }
  }
  const SRec* __restrict__ recs = bv.srecs + it.rec_off;
  const double* pts = bv.pt_state[st.sel] + (size_t)wd.pt_off * 3;
  const double* DL = bv.DL + (size_t)wd.pt_off * 9;
  const int mrow = lane & 15, mk = lane >> 4;
  using std::integral_constant;

  auto body = [&](auto lmc, auto psc) __attribute__((always_inline)) {
    constexpr int LM = decltype(lmc)::value, PS = decltype(psc)::value;   // landmarks per chunk, pose lanes
    constexpr int KS = 3 * LM + 1;                                        // LDS row stride (doubles): odd, conflict-free MFMA reads
    constexpr int KST = (3 * LM) / 4;                                     // k steps per chunk
    static_assert(LM * PS <= 64 && (3 * LM) % 4 == 0 && (POSE_ONLY || ((6 * PS + 15) / 16) * 16 * KS <= kImage), "chunk mapping");
    const int l = lane / PS, s = lane - l * PS;
    const bool lane_on = LM * PS == 64 || l < LM;
    f64x4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double bacc[3][3][3];   // BLK: [tile row][tile column][four-block instruction], one entry per lane each
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int q = 0; q < 3; ++q) bacc[a][b][q] = 0.0;
    double csum[6] = {0, 0, 0, 0, 0, 0};
    double H[21], hb[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) hb[k] = 0.0;
    if (kSchur && PS < 8) {
      // image rows past the pose lanes (up to the end of the last tile): nobody writes them
      for (int idx = lane; idx < (((6 * PS + 15) / 16) * 16 - 6 * PS) * KS; idx += 64) shA[6 * PS * KS + idx] = 0.0;
    }

    // Software pipeline over the chunks: the data of chunk c+1 are requested right after chunk c's operands are parked in LDS,
    // so they are in flight during chunk c's MFMA phase, and the record of chunk c+2 with them.  Every load is unconditional
    // on a clamped index (a load inside a divergent branch is waited for at the end of the branch); validity is applied
    // when the values are used.
    struct Dat { double2 ex[2]; double2 ey[2]; double X[3]; double dl[9]; };
    const int last_rec = it.n_lm - 1;
    const size_t last_edge = (size_t)wd.edge_off + (size_t)max(wd.E - 1, 0);
    auto load_rec = [&](int c0, int4& ra, int4& rb) {
      const int4* src = reinterpret_cast<const int4*>(recs + min(c0 + l, last_rec));
      ra = src[0]; rb = src[1];          // {lm, e_first, x_lo, x_hi} {y_lo, y_hi, flags, pad}
    };
    auto slot_of = [&](unsigned lo, unsigned hi) { return (((s < 4) ? lo : hi) >> (8 * (s & 3))) & 0xffu; };
    auto edge_of = [&](const int4& ra, unsigned o) { return min((size_t)wd.edge_off + (size_t)(ra.y + (o != kAbsent ? (int)o : 0)), last_edge); };
    auto load_dat = [&](const int4& ra, const int4& rb, Dat& d) {
      const double2* src = reinterpret_cast<const double2*>(bv.e_rec + edge_of(ra, slot_of((unsigned)ra.z, (unsigned)ra.w)) * 4);
      d.ex[0] = src[0]; d.ex[1] = src[1];
      if (!SYM) {
        const double2* sy = reinterpret_cast<const double2*>(bv.e_rec + edge_of(ra, slot_of((unsigned)rb.x, (unsigned)rb.y)) * 4);
        d.ey[0] = sy[0]; d.ey[1] = sy[1];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) d.X[k] = pts[(size_t)ra.x * 3 + k];
      if (do_schur) {
#pragma unroll
        for (int k = 0; k < 9; ++k) d.dl[k] = DL[(size_t)ra.x * 9 + k];
      }
    };
    // rows of W F of the lane's edge on one side of the item (side 0: row poses, 1: column poses) -> the side's LDS image
    auto side_rows = [&](int side, bool present, const int4& ra, unsigned o, const double2* er, const Dat& d, double* img) __attribute__((always_inline)) {
      const double* ps = shPose + (side * 8 + s) * kPoseRec;
      double qt[7], cam[5], Rm[9];
#pragma unroll
      for (int k = 0; k < 7; ++k) qt[k] = ps[k];
#pragma unroll
      for (int k = 0; k < 5; ++k) cam[k] = ps[7 + k];
#pragma unroll
      for (int k = 0; k < 9; ++k) Rm[k] = ps[12 + k];
      const double rec[4] = {er[0].x, er[0].y, er[1].x, er[1].y};
      double Xc[3], Q[6], g[3], rho0;
      win_edge_core<KB8>(wd, bv, edge_of(ra, o), rec, qt, cam, Rm, d.X, Xc, Q, g, rho0);
      // an empty slot computes on another edge's data: its result is discarded here (select, not multiply: it may be NaN)
#pragma unroll
      for (int k = 0; k < 6; ++k) Q[k] = present ? Q[k] : 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = present ? g[k] : 0.0;
      if (SYM && do_hpp && side == 0) dev::core_pose_side<KB8>(Xc, Q, g, H, hb);
      if (do_schur) {
        double WF[18];
        dev::core_WF<KB8>(Xc, Q, Rm, d.dl, WF);
        double* row = img + (6 * s) * KS + 3 * l;
        if (lane_on) {
#pragma unroll
          for (int r = 0; r < 6; ++r) { row[r * KS + 0] = WF[r * 3]; row[r * KS + 1] = WF[r * 3 + 1]; row[r * KS + 2] = WF[r * 3 + 2]; }
        }
        if (SYM) {
#pragma unroll
          for (int r = 0; r < 6; ++r) csum[r] += WF[r * 3] * d.dl[6] + WF[r * 3 + 1] * d.dl[7] + WF[r * 3 + 2] * d.dl[8];
        }
      }
    };
    // (always inlined: as a call, in the fisheye instantiation, every accumulator it touches by reference would live in scratch memory)
    auto park = [&](int c0, const int4& ra, const int4& rb, const Dat& d) __attribute__((always_inline)) {
      const bool valid = lane_on && (c0 + l) < it.n_lm;
      const unsigned xo = valid ? slot_of((unsigned)ra.z, (unsigned)ra.w) : kAbsent;
      wave_sync();   // the previous chunk's MFMA reads are done
      side_rows(0, xo != kAbsent, ra, xo, d.ex, d, shA);
      if (!SYM) {
        const unsigned yo = valid ? slot_of((unsigned)rb.x, (unsigned)rb.y) : kAbsent;
        side_rows(1, yo != kAbsent, ra, yo, d.ey, d, shB);
      }
    };
    // The tile counts are compile-time constants inside each instantiation (dispatched once per chunk): with run-time tile tests
    // every MFMA and every operand read sat behind its own scalar branch.
    auto multiply_t = [&](auto txc, auto tyc) {
      constexpr int TXc = decltype(txc)::value, TYc = decltype(tyc)::value;
      const double* imgB = SYM ? shA : shB;
#pragma unroll
      for (int ks = 0; ks < KST; ++ks) {
        double a[3], b[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          a[t] = (t < TXc) ? shA[(16 * t + mrow) * KS + 4 * ks + mk] : 0.0;
          b[t] = SYM ? a[t] : ((t < TYc) ? imgB[(16 * t + mrow) * KS + 4 * ks + mk] : 0.0);
        }
#pragma unroll
        for (int ti = 0; ti < 3; ++ti)
#pragma unroll
          for (int tj = SYM ? ti : 0; tj < 3; ++tj)
            if (ti < TXc && tj < TYc) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);   // operands of two k-steps in flight at most (the prefetched chunk needs the registers)
      }
    };
    // BLK: the multiply of an item of NX row poses (see above k_schur_fused).  The row offsets of the turned and the single-block-row
    // operands are the lane's own for the whole item; per k step they cost one LDS read each beside the a[t] of the tiles.
    const int off_a = mrow * KS + mk, off_s1 = ((mrow + 4) & 15) * KS + mk, off_s2 = ((mrow + 8) & 15) * KS + mk, off_c = (lane & 3) * KS + mk;
    auto multiply_b = [&](auto nxc) {
      constexpr int NX = decltype(nxc)::value, TXc = (6 * NX + 15) / 16, LL = schur_live_blocks(NX, TXc - 1);   // only the last tile is ragged
#pragma unroll
      for (int ks = 0; ks < KST; ++ks) {
        double a[3], s1[3], s2[3], cb[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const bool full = t < TXc && (t < TXc - 1 || LL == 4);
          a[t] = (t < TXc) ? shA[16 * t * KS + off_a + 4 * ks] : 0.0;
          s1[t] = full ? shA[16 * t * KS + off_s1 + 4 * ks] : 0.0;
          s2[t] = full ? shA[16 * t * KS + off_s2 + 4 * ks] : 0.0;
          cb[t] = (LL < 4 && t < LL) ? shA[(16 * (TXc - 1) + 4 * t) * KS + off_c + 4 * ks] : 0.0;
        }
#pragma unroll
        for (int ti = 0; ti < TXc; ++ti)
#pragma unroll
          for (int tj = ti; tj < TXc; ++tj) {
            if (tj == TXc - 1 && LL < 4) {
#pragma unroll
              for (int c = 0; c < LL; ++c) bacc[ti][tj][c] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[ti], cb[c], bacc[ti][tj][c], 0, 0, 0);
            } else if (ti == tj) {
              bacc[ti][ti][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[ti], a[ti], bacc[ti][ti][0], 0, 0, 0);
              bacc[ti][ti][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[ti], s1[ti], bacc[ti][ti][1], 0, 0, 0);
              bacc[ti][ti][2] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[ti], s2[ti], bacc[ti][ti][2], 0, 0, 0);
            } else {
              acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], a[tj], acc[ti][tj], 0, 0, 0);
            }
          }
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);   // as in multiply_t
      }
    };
    // BLK: the contributions of the item, the entries multiply_t's tiles would have stored and no others.  Pose pairs sa < sb only
    // have blocks with block row <= block column (schur_plan.h marks pair (sa, sb) live for sa <= sb only); a diagonal pair's 6 x 6
    // contribution is stored in full wherever both (r, c) and (c, r) lie in one diagonal tile, as the tile stored it.
    auto store_b = [&](auto nxc) {
      constexpr int NX = decltype(nxc)::value, TXc = (6 * NX + 15) / 16, LL = schur_live_blocks(NX, TXc - 1);
      const int bi = lane >> 4, bq = (lane >> 2) & 3, bj = lane & 3;
      // entry (R, C), R <= C; mirrored: an off-diagonal block of a diagonal tile also fills (C, R) of a diagonal pose pair
      auto put = [&](int R, int C, double v, bool mirrored) {
        const int sa = R / 6, rr = R - 6 * sa, sb = C / 6, cc = C - 6 * sb;
        const int slot = shP[sa * 8 + sb];
        if (slot >= 0) {
          bv.contrib[(size_t)slot * 36 + rr * 6 + cc] = v;
          if (mirrored && sa == sb) bv.contrib[(size_t)slot * 36 + cc * 6 + rr] = v;
        }
      };
#pragma unroll
      for (int ti = 0; ti < TXc; ++ti)
#pragma unroll
        for (int tj = ti; tj < TXc; ++tj) {
          if (tj == TXc - 1 && LL < 4) {
#pragma unroll
            for (int c = 0; c < LL; ++c) {
              const int R = 16 * ti + 4 * bq + bi, C = 16 * tj + 4 * c + bj;
              if (ti < tj || bq == c) {
                const int sa = R / 6, sb = C / 6, slot = shP[sa * 8 + sb];   // as the tile: (r, c) where the lane holds it
                if (slot >= 0) bv.contrib[(size_t)slot * 36 + (R - 6 * sa) * 6 + (C - 6 * sb)] = bacc[ti][tj][c];
              } else if (bq < c) {
                put(R, C, bacc[ti][tj][c], true);
              }
            }
          } else if (ti == tj) {
            const int R = 16 * ti + 4 * bq + bi;
            {
              const int C = 16 * ti + 4 * bq + bj;
              const int sa = R / 6, sb = C / 6, slot = shP[sa * 8 + sb];
              if (slot >= 0) bv.contrib[(size_t)slot * 36 + (R - 6 * sa) * 6 + (C - 6 * sb)] = bacc[ti][ti][0];
            }
            {
              const int C = 16 * ti + 4 * ((bq + 1) & 3) + bj;   // block (3, 0): the mirror image of (0, 3)
              put(bq == 3 ? C : R, bq == 3 ? R : C, bacc[ti][ti][1], true);
            }
            if (bq < 2) put(R, 16 * ti + 4 * (bq + 2) + bj, bacc[ti][ti][2], true);
          } else {
            const int C = 16 * tj + (lane & 15);
            const int sb = C / 6, cc = C - 6 * sb;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int R = 16 * ti + (lane >> 4) + 4 * reg;
              const int sa = R / 6, rr = R - 6 * sa;
              const int slot = shP[sa * 8 + sb];
              if (slot >= 0) bv.contrib[(size_t)slot * 36 + rr * 6 + cc] = acc[ti][tj][reg];
            }
          }
        }
    };
    auto multiply_cross = [&]() {
      // Cross items that come here (fisheye, or more than 4 column poses: parts b of tracks with 13+ observers) keep run-time tile
      // tests: nine instantiations cost registers for no gain.  Pinhole cross items of at most 4 column poses -- every cross item of
      // the headline window -- take cross_pairs() below: TX = 3, TY = 1 or 2 at compile time.
#pragma unroll
      for (int ks = 0; ks < KST; ++ks) {
        double a[3], b[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          a[t] = (t < TX) ? shA[(16 * t + mrow) * KS + 4 * ks + mk] : 0.0;
          b[t] = (t < TY) ? shB[(16 * t + mrow) * KS + 4 * ks + mk] : 0.0;
        }
#pragma unroll
        for (int ti = 0; ti < 3; ++ti)
#pragma unroll
          for (int tj = 0; tj < 3; ++tj)
            if (ti < TX && tj < TY) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
      }
    };
    int4 rc0, rc1, rn0, rn1;
    Dat d;
    load_rec(0, rc0, rc1);
    load_rec(LM, rn0, rn1);
    load_dat(rc0, rc1, d);
    wave_sync();   // the staged poses are visible
    // The chunk loop is instantiated per tile count (dispatched ONCE per item): a dispatch inside the loop makes the compiler
    // reconcile the register assignment of the accumulators at every merge (dozens of 64-bit moves per chunk).
    // (BLK: per number of row poses, so that the block list of the ragged last tile is a compile-time constant too)
    auto chunk_loop = [&](auto txc) {
      for (int c0 = 0; c0 < it.n_lm; c0 += LM) {
        park(c0, rc0, rc1, d);                 // edge descriptions, W F rows of chunk c0 -> LDS (consumes d)
        wave_sync();
        rc0 = rn0; rc1 = rn1;                  // loaded one iteration ago
        load_dat(rc0, rc1, d);                 // chunk c0 + 1: in flight during the MFMAs below
        load_rec(c0 + 2 * LM, rn0, rn1);
        if (do_schur) {
          if constexpr (BLK && decltype(txc)::value > 0) multiply_b(txc);   // (txc: NX)
          else if (SYM) multiply_t(txc, txc);
          else multiply_cross();
        }
      }
      if constexpr (BLK && decltype(txc)::value > 0) store_b(txc);
    };
    if (SYM && do_schur) {   // TX == TY
      if constexpr (BLK) {
        if constexpr (PS == 8) {
          if (nx >= 8) chunk_loop(integral_constant<int, 8>{});
          else if (nx == 7) chunk_loop(integral_constant<int, 7>{});
          else chunk_loop(integral_constant<int, 6>{});
        } else if constexpr (PS == 5) {
          chunk_loop(integral_constant<int, 5>{});
        } else {
          if (nx >= 4) chunk_loop(integral_constant<int, 4>{});
          else if (nx == 3) chunk_loop(integral_constant<int, 3>{});
          else if (nx == 2) chunk_loop(integral_constant<int, 2>{});
          else chunk_loop(integral_constant<int, 1>{});
        }
      } else {
        if (PS > 5 && TX == 3) chunk_loop(integral_constant<int, 3>{});
        else if (PS > 2 && TX == 2) chunk_loop(integral_constant<int, 2>{});
        else chunk_loop(integral_constant<int, 1>{});
      }
    } else {
      chunk_loop(integral_constant<int, 0>{});
    }
    wave_sync();
    if (do_schur) {
      // contributions: lane holds D[row = (lane >> 4) + 4 reg][col = lane & 15] of each tile  (BLK: stored by store_b)
#pragma unroll
      for (int ti = 0; ti < (BLK ? 0 : 3); ++ti)
#pragma unroll
        for (int tj = SYM ? ti : 0; tj < 3; ++tj) {
          if (ti < TX && tj < TY) {
            const int C = 16 * tj + (lane & 15);
            const int sb = C / 6, cc = C - 6 * sb;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int R = 16 * ti + (lane >> 4) + 4 * reg;
              const int sa = R / 6, rr = R - 6 * sa;
              const int slot = shP[sa * 8 + sb];
              if (slot >= 0) bv.contrib[(size_t)slot * 36 + rr * 6 + cc] = acc[ti][tj][reg];
            }
          }
        }
      if (SYM) {
        // rhs term of row pose s: sum over the landmark lanes in fixed order
        if (lane_on) {
#pragma unroll
          for (int r = 0; r < 6; ++r) shA[l * (6 * PS) + 6 * s + r] = csum[r];
        }
        wave_sync();
        if (lane < 6 * PS) {
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < LM; ++k) v += shA[k * (6 * PS) + lane];
          const int sa = lane / 6;
          const int slot = shP[64 + sa];
          if (slot >= 0) bv.ccontrib[(size_t)slot * 6 + (lane - 6 * sa)] = v;
        }
        wave_sync();
      }
    }
    if (SYM && do_hpp) {
      // Hpp / b_p of row pose s: sum over the landmark lanes in fixed order (two halves through the image buffer)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int k0 = half * 14, nk = half ? 13 : 14;
        wave_sync();
#pragma unroll
        for (int k = 0; k < 14; ++k) {
          const int kk = k0 + k;
          if (k < nk) shA[k * 64 + lane] = (kk < 21) ? H[kk < 21 ? kk : 0] : hb[(kk - 21) < 0 ? 0 : ((kk - 21) > 5 ? 5 : (kk - 21))];
        }
        wave_sync();
        for (int o = lane; o < PS * nk; o += 64) {
          const int k = o / PS, sa = o - k * PS;
          const int slot = shP[64 + sa];
          if (slot >= 0) {
            double v = 0.0;
#pragma unroll
            for (int ll = 0; ll < LM; ++ll) v += shA[k * 64 + ll * PS + sa];
            bv.hcontrib[(size_t)slot * 27 + k0 + k] = v;
          }
        }
      }
    }
  };
  // Pinhole cross items of at most 4 column poses (part b of a 9-12-observer track; on the headline window all of them: 85 items,
  // 465 chunks, an edge in 0.29 of the 8 x 8 column lane slots).  The row side stays one 8 x 8 pass per chunk; the column side is ONE
  // 16 x 4 pass for a PAIR of chunks: lane (l, s) = landmark l of 16, column slot s of 4, rows 6 s + r of the 24 x 49 column image (in the 48 x 25 doubles of shB), whose
  // columns 0..23 belong to the first chunk of the pair and 24..47 to the second.  The k steps of a chunk read the same (landmark,
  // component) columns in the same order as with one 8 x 8 column pass per chunk, so every Schur product keeps its bits.  TX is 3 (part
  // a of such a track has 8 poses), TY 1 or 2: the loop is instantiated for the two values of TY and dispatched once per item.
  auto cross_pairs = [&](auto tyc) __attribute__((always_inline)) {
    constexpr int TYc = decltype(tyc)::value;
    constexpr int KS = 3 * kSiLm + 1, KSB = 3 * 16 + 1, KST = (3 * kSiLm) / 4;
    static_assert(16 * TYc <= 32 && kSiRows * KS <= sizeof(shA) / sizeof(double) && 24 * KSB <= sizeof(shB) / sizeof(double), "image sizes");
    const int l = lane >> 3, s = lane & 7;      // row pass
    const int lc = lane >> 2, sc = lane & 3;    // column pass
    f64x4 acc[3][TYc];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < TYc; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};

    // Software pipeline as in body(): row record two chunks ahead and row data one chunk ahead; the column records two PAIRS ahead and
    // the column data of the next pair requested before the MFMAs of a pair's second chunk.  Every load unconditional on a clamped index.
    struct SDat { double2 e[2]; double X[3]; double dl[9]; };
    const int last_rec = it.n_lm - 1;
    const size_t last_edge = (size_t)wd.edge_off + (size_t)max(wd.E - 1, 0);
    auto edge_of = [&](const int4& ra, unsigned o) { return min((size_t)wd.edge_off + (size_t)(ra.y + (o != kAbsent ? (int)o : 0)), last_edge); };
    auto row_slot = [&](const int4& ra) { return (unsigned)((((unsigned long long)(unsigned)ra.w << 32) | (unsigned)ra.z) >> (8 * s)) & 0xffu; };
    auto col_slot = [&](const int4& rb) { return ((unsigned)rb.x >> (8 * sc)) & 0xffu; };   // slots 0..3: y_lo
    auto load_row_rec = [&](int c0, int4& ra) { ra = *reinterpret_cast<const int4*>(recs + min(c0 + l, last_rec)); };
    auto load_col_rec = [&](int p0, int4& ra, int4& rb) {
      const int4* src = reinterpret_cast<const int4*>(recs + min(p0 + lc, last_rec));
      ra = src[0]; rb = src[1];
    };
    auto load_dat = [&](const int4& ra, unsigned o, SDat& d) {
      const double2* src = reinterpret_cast<const double2*>(bv.e_rec + edge_of(ra, o) * 4);
      d.e[0] = src[0]; d.e[1] = src[1];
#pragma unroll
      for (int k = 0; k < 3; ++k) d.X[k] = pts[(size_t)ra.x * 3 + k];
#pragma unroll
      for (int k = 0; k < 9; ++k) d.dl[k] = DL[(size_t)ra.x * 9 + k];
    };
    // rows of W F of one edge -> six rows of an image (as side_rows of body())
    auto wf_rows = [&](const double* ps, bool present, size_t ge, const SDat& d, double* row, int ks) __attribute__((always_inline)) {
      double qt[7], cam[5], Rm[9];
#pragma unroll
      for (int k = 0; k < 7; ++k) qt[k] = ps[k];
#pragma unroll
      for (int k = 0; k < 5; ++k) cam[k] = ps[7 + k];
#pragma unroll
      for (int k = 0; k < 9; ++k) Rm[k] = ps[12 + k];
      const double rec[4] = {d.e[0].x, d.e[0].y, d.e[1].x, d.e[1].y};
      double Xc[3], Q[6], g[3], rho0;
      win_edge_core<KB8>(wd, bv, ge, rec, qt, cam, Rm, d.X, Xc, Q, g, rho0);
      // an empty slot computes on another edge's data: its result is discarded here (select, not multiply: it may be NaN)
#pragma unroll
      for (int k = 0; k < 6; ++k) Q[k] = present ? Q[k] : 0.0;
      double WF[18];
      dev::core_WF<KB8>(Xc, Q, Rm, d.dl, WF);
#pragma unroll
      for (int r = 0; r < 6; ++r) { row[r * ks + 0] = WF[r * 3]; row[r * ks + 1] = WF[r * 3 + 1]; row[r * ks + 2] = WF[r * 3 + 2]; }
    };
    auto row_pass = [&](int c0, const int4& ra, const SDat& d) __attribute__((always_inline)) {
      const unsigned o = (c0 + l) < it.n_lm ? row_slot(ra) : kAbsent;
      wf_rows(shPose + s * kPoseRec, o != kAbsent, edge_of(ra, o), d, shA + (6 * s) * KS + 3 * l, KS);
    };
    auto col_pass = [&](int p0, const int4& ra, const int4& rb, const SDat& d) __attribute__((always_inline)) {
      const unsigned o = (p0 + lc) < it.n_lm ? col_slot(rb) : kAbsent;
      wf_rows(shPose + (8 + sc) * kPoseRec, o != kAbsent, edge_of(ra, o), d, shB + (6 * sc) * KSB + 3 * lc, KSB);
    };
    // the k steps of one chunk: A columns 0..23, B columns cb..cb + 23 (cb = 0 / 24: first / second chunk of the pair)
    auto multiply = [&](int cb) __attribute__((always_inline)) {
#pragma unroll
      for (int ks = 0; ks < KST; ++ks) {
        double a[3], b[TYc];
#pragma unroll
        for (int t = 0; t < 3; ++t) a[t] = shA[(16 * t + mrow) * KS + 4 * ks + mk];
#pragma unroll
        for (int t = 0; t < TYc; ++t) b[t] = shB[min(16 * t + mrow, 23) * KSB + cb + 4 * ks + mk];   // (rows 24..31: columns of D nobody stores)
#pragma unroll
        for (int ti = 0; ti < 3; ++ti)
#pragma unroll
          for (int tj = 0; tj < TYc; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);   // operands of two k-steps in flight at most (the prefetched chunks need the registers)
      }
    };
    int4 rc, rn, cc0, cc1, cn0, cn1;
    SDat rd, cd;
    load_row_rec(0, rc);
    load_col_rec(0, cc0, cc1);
    load_row_rec(kSiLm, rn);
    load_col_rec(2 * kSiLm, cn0, cn1);
    load_dat(rc, row_slot(rc), rd);
    load_dat(cc0, col_slot(cc1), cd);
    wave_sync();   // the staged poses are visible
    int p0 = 0;
    for (; p0 + kSiLm < it.n_lm; p0 += 2 * kSiLm) {     // pairs of chunks p0, p0 + 8
      wave_sync();                                      // the previous chunk's MFMA reads are done
      col_pass(p0, cc0, cc1, cd);                       // both chunks' column rows -> shB (consumes cd)
      row_pass(p0, rc, rd);                             // (consumes rd)
      wave_sync();
      rc = rn;
      load_dat(rc, row_slot(rc), rd);                   // rows of chunk p0 + 8: in flight during the MFMAs below
      load_row_rec(p0 + 2 * kSiLm, rn);
      multiply(0);
      wave_sync();
      row_pass(p0 + kSiLm, rc, rd);
      wave_sync();
      rc = rn; cc0 = cn0; cc1 = cn1;
      load_dat(rc, row_slot(rc), rd);                   // rows of chunk p0 + 16 and columns of the pair that starts there
      load_dat(cc0, col_slot(cc1), cd);
      load_row_rec(p0 + 3 * kSiLm, rn);
      load_col_rec(p0 + 4 * kSiLm, cn0, cn1);
      multiply(3 * kSiLm);
    }
    if (p0 < it.n_lm) {                                 // an odd number of chunks: the last one alone (columns 24..47 are written, not read)
      wave_sync();
      col_pass(p0, cc0, cc1, cd);
      row_pass(p0, rc, rd);
      wave_sync();
      multiply(0);
    }
    // contributions: lane holds D[row = (lane >> 4) + 4 reg][col = lane & 15] of each tile
#pragma unroll
    for (int ti = 0; ti < 3; ++ti)
#pragma unroll
      for (int tj = 0; tj < TYc; ++tj) {
        const int C = 16 * tj + (lane & 15);
        const int sb = C / 6, cc = C - 6 * sb;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int R = 16 * ti + (lane >> 4) + 4 * reg;
          const int sa = R / 6, rr = R - 6 * sa;
          const int slot = shP[sa * 8 + sb];
          if (slot >= 0) bv.contrib[(size_t)slot * 36 + rr * 6 + cc] = acc[ti][tj][reg];
        }
      }
  };
  if constexpr (!SYM && !KB8) {
    if (nx > 5 && ny <= 4) {
      if (ny <= 2) cross_pairs(integral_constant<int, 1>{}); else cross_pairs(integral_constant<int, 2>{});
      return;
    }
  }
  if constexpr (SYM && !KB8) {
    if (nx <= 4) body(integral_constant<int, 16>{}, integral_constant<int, 4>{});
    else if (nx == 5) body(integral_constant<int, 12>{}, integral_constant<int, 5>{});
    else body(integral_constant<int, kSiLm>{}, integral_constant<int, 8>{});
  } else {
    body(integral_constant<int, kSiLm>{}, integral_constant<int, 8>{});
  }
}
}  // namespace osh
