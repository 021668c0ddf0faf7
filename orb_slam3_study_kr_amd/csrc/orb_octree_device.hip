// orb_octree_device.hip -- ORBextractor::DistributeOctTree (src/ORBextractor.cc:480-779) on MI355X (gfx950) for a batch of
// (frame, level) lists: the quadtree that thins the FAST candidates of a level to about N keypoints.  The statements and the
// array form of the list are those of orb_octree.h; this file is the parallel walk.
//
// octree_run is the one way to the kernel: lists up, k_octree on candidates that are on the device, counts down, the kept indices left
// there.  osh_orb_octree_distribute stages host candidates for it and downloads the indices; osh_orb_extract (orb_extract_device.hip)
// hands it the detector's emit buffer.
//
// osh_orb_octree_distribute, k_octree: one workgroup of 8 wavefronts per list, the list in LDS.
//   nodes    two copies of the list (box as 4 x 16 bits, key run as begin | buffer bit, count): a round reads one and writes the other;
//   keys     a permutation of the input indices as 16-bit values in two buffers.  A node's run is in the buffer its bit names; a
//            division writes the four runs of the children into the same range of the other buffer, so a node that is not divided
//            moves no key.  With the coordinates, the buffers are in LDS up to kOctLdsKeys keys and in global memory beyond;
//   round    proc (round A: a prefix sum over "more than one key"; round B: a rank sort of E by oct_sort_key, walked from the back),
//            one wavefront per node of proc counting its quadrants with ballots, a prefix sum over "non-empty children" that gives
//            every child its place (and, in round B, the break), a prefix sum over the undivided nodes for theirs, then one wavefront
//            per divided node again to write children and keys.  No lane walks a list.
//   winners  one wavefront per node: the maximum of oct_winner_key over its run.
// Every loop is counted: rounds by kOctMaxRounds (orb_octree.h derives it), node loops by the list length, key loops by the run
// length, the scans by kOctPer entries per thread.  A list that reaches kOctMaxRounds, or whose list would outgrow kOctMaxNodes, comes
// back with a status and is not continued.
#include "common.h"
#include "orb_extract.h"
#include "orb_octree.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

static_assert(kOctMaxFeatures == OSH_OCTREE_MAX_FEATURES && kOctMaxKeys == OSH_OCTREE_MAX_CANDIDATES && kOctMaxRoots == OSH_OCTREE_MAX_ROOTS &&
              kOctMaxSide == OSH_FAST_MAX_SIDE, "orb_octree.h and include/orbslam3_hip.h name the same limits");
static_assert(kOctOk == OSH_OK && kOctInvalid == OSH_ERR_INVALID && kOctUnsupported == OSH_ERR_UNSUPPORTED, "codes of oct_validate_list");

constexpr int kOctBlock = 512;                             // 8 wavefronts
constexpr int kOctWaves = kOctBlock / 64;
constexpr int kOctPer = (kOctMaxNodes + kOctBlock - 1) / kOctBlock;   // list entries per thread of a scan: 5
constexpr int kOctLdsKeys = 2048;                          // keys of a list that stay in LDS
constexpr unsigned kOctBufBit = 0x80000000u;
constexpr unsigned short kOctGone = 0xffff;

// dynamic LDS, in bytes from its start
constexpr size_t kOctOffBox = 0;                                                           // ushort4 [2][kOctMaxNodes]
constexpr size_t kOctOffSeg = kOctOffBox + 2 * sizeof(ushort4) * kOctMaxNodes;             // uint2   [2][kOctMaxNodes]
constexpr size_t kOctOffCnt = kOctOffSeg + 2 * sizeof(uint2) * kOctMaxNodes;               // uint4   [kOctMaxNodes]; the sort keys before
constexpr size_t kOctOffPre = kOctOffCnt + sizeof(uint4) * kOctMaxNodes;                   // unsigned [kOctMaxNodes]
constexpr size_t kOctOffProc = kOctOffPre + sizeof(unsigned) * kOctMaxNodes;               // unsigned short [kOctMaxNodes]
constexpr size_t kOctOffE = kOctOffProc + sizeof(unsigned short) * kOctMaxNodes;           // unsigned short [kOctMaxNodes]
constexpr size_t kOctOffNewPos = kOctOffE + sizeof(unsigned short) * kOctMaxNodes;         // unsigned short [kOctMaxNodes]
constexpr size_t kOctOffMisc = kOctOffNewPos + sizeof(unsigned short) * kOctMaxNodes;      // int [64]: wave sums, round results, roots
constexpr size_t kOctOffRoots = kOctOffMisc + sizeof(int) * 64;                            // int [2][kOctMaxRoots]
constexpr size_t kOctOffKeyX = kOctOffRoots + 2 * sizeof(int) * kOctMaxRoots;              // float [kOctLdsKeys]
constexpr size_t kOctOffKeyY = kOctOffKeyX + sizeof(float) * kOctLdsKeys;
constexpr size_t kOctOffPerm = kOctOffKeyY + sizeof(float) * kOctLdsKeys;                  // unsigned short [2][kOctLdsKeys]
constexpr size_t kOctLdsBytes = kOctOffPerm + 2 * sizeof(unsigned short) * kOctLdsKeys;
static_assert(kOctLdsBytes <= 160 * 1024, "one workgroup's LDS on gfx950");
static_assert(kOctMaxNodes < kOctGone && kOctPer * kOctBlock >= kOctMaxNodes && 4 * kOctMaxNodes < 65536, "16-bit positions and packed prefix sums");

struct OctView {
  const OctListDev* lists;
  const float2* xy;
  const float* response;
  unsigned short* work;
  int* out_index; int* out_count; int* out_status;
};

// Exclusive prefix sum over i in [0, count) of get(i), entries [tid * kOctPer, (tid + 1) * kOctPer) per thread: put(i, sum before i,
// get(i)) for every i, the total returned.  Every thread of the block calls it; it ends with a barrier.
template <class Get, class Put>
__device__ int oct_scan(int count, int* sh_wave, Get get, Put put) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int val[kOctPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kOctPer; ++j) { const int i = tid * kOctPer + j; val[j] = i < count ? get(i) : 0; sum += val[j]; }
  int incl = sum;
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) { const int up = __shfl_up(incl, step); if (lane >= step) incl += up; }
  if (lane == 63) sh_wave[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kOctWaves; ++w) { const int s = sh_wave[w]; total += s; if (w < wave) before += s; }
  int run = before + incl - sum;
#pragma unroll
  for (int j = 0; j < kOctPer; ++j) { const int i = tid * kOctPer + j; if (i < count) { put(i, run, val[j]); run += val[j]; } }
  __syncthreads();
  return total;
}

__device__ inline OctBox oct_unpack(ushort4 b) { return {(int)b.x, (int)b.y, (int)b.z, (int)b.w}; }
__device__ inline ushort4 oct_pack(const OctBox& b) { return make_ushort4((unsigned short)b.ulx, (unsigned short)b.urx, (unsigned short)b.uly, (unsigned short)b.bry); }

__global__ __launch_bounds__(kOctBlock) void k_octree(OctView v) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  ushort4* const box = reinterpret_cast<ushort4*>(lds + kOctOffBox);       // [buffer * kOctMaxNodes + position]
  uint2* const seg = reinterpret_cast<uint2*>(lds + kOctOffSeg);           // x: begin | buffer bit, y: count
  uint4* const cnt = reinterpret_cast<uint4*>(lds + kOctOffCnt);           // [t] keys per quadrant of proc[t]
  unsigned long long* const sort_key = reinterpret_cast<unsigned long long*>(lds + kOctOffCnt);
  unsigned* const pre = reinterpret_cast<unsigned*>(lds + kOctOffPre);     // [t] non-empty children before t | children with > 1 key before t << 16
  unsigned short* const proc = reinterpret_cast<unsigned short*>(lds + kOctOffProc);
  unsigned short* const E = reinterpret_cast<unsigned short*>(lds + kOctOffE);
  unsigned short* const newpos = reinterpret_cast<unsigned short*>(lds + kOctOffNewPos);
  int* const sh_wave = reinterpret_cast<int*>(lds + kOctOffMisc);          // [kOctWaves]
  int* const sh_round = sh_wave + 16;                                      // P, C, M of a round
  int* const root_count = reinterpret_cast<int*>(lds + kOctOffRoots);
  int* const root_begin = root_count + kOctMaxRoots;

  const OctListDev L = v.lists[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long lt = (1ull << lane) - 1;
  const int n = L.n, N = L.N;
  if (n == 0) {   // no root has a key: the list is empty and does not grow
    if (tid == 0) { v.out_count[blockIdx.x] = 0; v.out_status[blockIdx.x] = OSH_OK; }
    return;
  }
  const bool in_lds = n <= kOctLdsKeys;
  const float2* const gxy = v.xy + L.key0;
  float* const kx = reinterpret_cast<float*>(lds + kOctOffKeyX);
  float* const ky = reinterpret_cast<float*>(lds + kOctOffKeyY);
  unsigned short* const perm0 = in_lds ? reinterpret_cast<unsigned short*>(lds + kOctOffPerm) : v.work + L.work0;
  unsigned short* const perm1 = perm0 + (in_lds ? kOctLdsKeys : n);
  const auto perm = [&](unsigned buffer) { return buffer ? perm1 : perm0; };
  const auto key_xy = [&](int k) { return in_lds ? make_float2(kx[k], ky[k]) : gxy[k]; };
  if (in_lds) for (int k = tid; k < n; k += kOctBlock) { const float2 p = gxy[k]; kx[k] = p.x; ky[k] = p.y; }
  __syncthreads();

  // ---- the roots: one wavefront per root passes over the keys twice, for its count and for its run in input order
  const int n_ini = oct_n_ini(L.W, L.H);
  const float hx = oct_hx(L.W, n_ini);
  const int chunks_n = (n + 63) / 64;
  for (int r = wave; r < n_ini; r += kOctWaves) {
    int c = 0;
    for (int ch = 0; ch < chunks_n; ++ch) {
      const int k = ch * 64 + lane;
      c += __popcll(__ballot(k < n && oct_root_of(key_xy(k).x, hx, n_ini) == r));
    }
    if (lane == 0) root_count[r] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int at = 0, S0 = 0;
    for (int r = 0; r < n_ini; ++r) {
      root_begin[r] = at;
      if (root_count[r]) { box[S0] = oct_pack(oct_root(hx, r, L.H)); seg[S0] = make_uint2((unsigned)at, (unsigned)root_count[r]); ++S0; }
      at += root_count[r];
    }
    sh_round[3] = S0;
  }
  __syncthreads();
  for (int r = wave; r < n_ini; r += kOctWaves) {
    int at = root_begin[r];
    for (int ch = 0; ch < chunks_n; ++ch) {
      const int k = ch * 64 + lane;
      const bool mine = k < n && oct_root_of(key_xy(k).x, hx, n_ini) == r;
      const unsigned long long b = __ballot(mine);
      if (mine) perm0[at + __popcll(b & lt)] = (unsigned short)k;
      at += __popcll(b);
    }
  }
  __syncthreads();

  int S = sh_round[3], cur = 0, m_E = 0, status = OSH_ERR_DEVICE;
  bool mode_b = false;
  for (int round = 0; round < kOctMaxRounds; ++round) {
    const ushort4* const cbox = box + cur * kOctMaxNodes;
    const uint2* const cseg = seg + cur * kOctMaxNodes;
    ushort4* const nbox = box + (cur ^ 1) * kOctMaxNodes;
    uint2* const nseg = seg + (cur ^ 1) * kOctMaxNodes;
    // 1. proc: the nodes this round divides, in the order it divides them
    int m;
    if (!mode_b) {
      m = oct_scan(S, sh_wave, [&](int p) { return cseg[p].y > 1u ? 1 : 0; }, [&](int p, int before, int val) { if (val) proc[before] = (unsigned short)p; });
    } else {
      m = m_E;
      for (int j = tid; j < m; j += kOctBlock) sort_key[j] = oct_sort_key((int)cseg[E[j]].y, (int)cbox[E[j]].x, j);
      __syncthreads();
      for (int j = tid; j < m; j += kOctBlock) {
        const unsigned long long mine = sort_key[j];
        int rank = 0;
        for (int i = 0; i < m; ++i) rank += sort_key[i] < mine ? 1 : 0;
        proc[m - 1 - rank] = E[j];   // walked from the back of the ascending order
      }
      __syncthreads();
    }
    // 2. the keys per quadrant of every node of proc
    for (int t = wave; t < m; t += kOctWaves) {
      const int p = proc[t];
      const uint2 sg = cseg[p];
      const int begin = (int)(sg.x & ~kOctBufBit), count = (int)sg.y;
      const unsigned short* const src = perm(sg.x >> 31) + begin;
      int mx, my;
      oct_mid(oct_unpack(cbox[p]), mx, my);
      int c0 = 0, c1 = 0, c2 = 0;
      const int chunks = (count + 63) / 64;
      for (int ch = 0; ch < chunks; ++ch) {
        const int k = ch * 64 + lane;
        int q = -1;
        if (k < count) { const float2 xy = key_xy(src[k]); q = oct_quadrant(xy.x, xy.y, mx, my); }
        c0 += __popcll(__ballot(q == 0)); c1 += __popcll(__ballot(q == 1)); c2 += __popcll(__ballot(q == 2));
      }
      if (lane == 0) cnt[t] = make_uint4((unsigned)c0, (unsigned)c1, (unsigned)c2, (unsigned)(count - c0 - c1 - c2));
    }
    if (tid == 0) { sh_round[0] = 0; sh_round[1] = 0; sh_round[2] = 0; }
    __syncthreads();
    // 3. where the children go; in round B, where the walk breaks
    const auto walks = [&](int t, int created_before) { return !mode_b || oct_b_walks(S, created_before, t, N); };
    oct_scan(m, sh_wave,
             [&](int t) {
               const uint4 c = cnt[t];
               const int nz = (c.x > 0) + (c.y > 0) + (c.z > 0) + (c.w > 0), multi = (c.x > 1) + (c.y > 1) + (c.z > 1) + (c.w > 1);
               return nz | (multi << 16);
             },
             [&](int t, int before, int val) {
               pre[t] = (unsigned)before;
               const int c_before = before & 0xffff, c_after = c_before + (val & 0xffff);
               if (walks(t, c_before) && (t == m - 1 || !walks(t + 1, c_after))) {   // the last node divided
                 sh_round[0] = t + 1; sh_round[1] = c_after; sh_round[2] = (before >> 16) + (val >> 16);
               }
             });
    const int P = sh_round[0], C = sh_round[1], M = sh_round[2];
    // 4. where the undivided nodes go
    for (int p = tid; p < S; p += kOctBlock) newpos[p] = 0;
    __syncthreads();
    for (int t = tid; t < P; t += kOctBlock) newpos[proc[t]] = 1;
    __syncthreads();
    const int Q = oct_scan(S, sh_wave, [&](int p) { return newpos[p] ? 0 : 1; },
                           [&](int p, int before, int val) { newpos[p] = val ? (unsigned short)(C + before) : kOctGone; });
    const int S_new = C + Q;
    if (S_new > kOctMaxNodes) { status = OSH_ERR_UNSUPPORTED; break; }   // cannot be: max(N + 3, 4 nIni) <= kOctMaxNodes
    // 5. the new list: children in reverse creation order, then the undivided nodes in their old order
    for (int p = tid; p < S; p += kOctBlock) {
      const int to = newpos[p];
      if (to != kOctGone) { nbox[to] = cbox[p]; nseg[to] = cseg[p]; }
    }
    for (int t = wave; t < P; t += kOctWaves) {
      const int p = proc[t];
      const uint2 sg = cseg[p];
      const unsigned buf = sg.x >> 31;
      const int begin = (int)(sg.x & ~kOctBufBit), count = (int)sg.y;
      const OctBox b = oct_unpack(cbox[p]);
      int mx, my;
      oct_mid(b, mx, my);
      const uint4 c = cnt[t];
      const int cq[4] = {(int)c.x, (int)c.y, (int)c.z, (int)c.w};
      int off[4];
      off[0] = 0; off[1] = cq[0]; off[2] = off[1] + cq[1]; off[3] = off[2] + cq[2];
      if (lane == 0) {
        int created = (int)(pre[t] & 0xffffu), multi = (int)(pre[t] >> 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!cq[q]) continue;
          const int to = C - 1 - created++;
          nbox[to] = oct_pack(oct_child(b, mx, my, q));
          nseg[to] = make_uint2((unsigned)(begin + off[q]) | ((buf ^ 1u) << 31), (unsigned)cq[q]);
          if (cq[q] > 1) E[multi++] = (unsigned short)to;
        }
      }
      const unsigned short* const src = perm(buf) + begin;
      unsigned short* const dst = perm(buf ^ 1u) + begin;
      int run[4] = {off[0], off[1], off[2], off[3]};
      const int chunks = (count + 63) / 64;
      for (int ch = 0; ch < chunks; ++ch) {
        const int k = ch * 64 + lane;
        int q = -1;
        unsigned short idx = 0;
        if (k < count) { idx = src[k]; const float2 xy = key_xy(idx); q = oct_quadrant(xy.x, xy.y, mx, my); }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const unsigned long long bq = __ballot(q == qq);
          if (q == qq) dst[run[qq] + __popcll(bq & lt)] = idx;
          run[qq] += __popcll(bq);
        }
      }
    }
    __syncthreads();
    // 6. the reference's exits
    const int S_prev = S;
    S = S_new; cur ^= 1; m_E = M;
    if (S >= N || S == S_prev) { status = OSH_OK; break; }
    if (!mode_b && S + 3 * M > N) mode_b = true;
  }

  // ---- per node, front to back, its strongest key
  if (status == OSH_OK) {
    const uint2* const cseg = seg + cur * kOctMaxNodes;
    const float* const resp = v.response + L.key0;
    for (int p = wave; p < S; p += kOctWaves) {
      const uint2 sg = cseg[p];
      const int count = (int)sg.y;
      const unsigned short* const src = perm(sg.x >> 31) + (sg.x & ~kOctBufBit);
      unsigned long long best = 0;
      const int chunks = (count + 63) / 64;
      for (int ch = 0; ch < chunks; ++ch) {
        const int k = ch * 64 + lane;
        if (k < count) { const unsigned idx = src[k]; const unsigned long long key = oct_winner_key(resp[idx], idx); best = key > best ? key : best; }
      }
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) { const unsigned long long o = __shfl_xor(best, step); best = o > best ? o : best; }
      if (lane == 0) v.out_index[L.out0 + p] = (int)oct_winner_index(best);
    }
  }
  if (tid == 0) { v.out_count[blockIdx.x] = status == OSH_OK ? S : 0; v.out_status[blockIdx.x] = status; }
}

struct OctreeState {
  StagedCall call;    // osh_orb_octree_distribute: the candidates in
  StagedCall run;     // octree_run: the lists in, [count | status | kept indices] out
  DevBuf work;        // the key buffers of the lists beyond kOctLdsKeys
  double ms[4] = {0, 0, 0, 0};
};

int octree_run(osh_orb_ctx* c, hipStream_t s, std::vector<OctListDev>& lists, const float2* xy, const float* response, std::vector<int>& count,
               std::vector<int>& status, const int** index) {
  const size_t n_lists = lists.size();
  OctreeState* st = orb_state<OctreeState>(c, kOrbAttachOctree);
  int device = 0;
  OSH_HIP(hipGetDevice(&device));
  OSH_TRY(allow_dynamic_lds(device, (int)kOctLdsBytes, k_octree));
  size_t out0 = 0, work0 = 0;
  for (OctListDev& l : lists) {
    l.out0 = (int)out0; l.work0 = (long long)work0;
    out0 += (size_t)std::min(l.n, kOctMaxNodes);
    if (l.n > kOctLdsKeys) work0 += 2 * (size_t)l.n;
  }
  Layout in, out;
  const auto s_lists = in.take<OctListDev>(n_lists);
  const auto o_count = out.take<int>(n_lists);
  const auto o_status = out.take<int>(n_lists);
  const size_t head_bytes = out.bytes;            // what comes back here; the indices stay
  const auto o_index = out.take<int>(out0);
  OSH_TRY(st->run.reserve(in, out));
  OSH_TRY(st->work.reserve(std::max<size_t>(work0, 1) * sizeof(unsigned short)));
  std::memcpy(s_lists.in(st->run.host_in()), lists.data(), sizeof(OctListDev) * n_lists);
  OSH_TRY(st->run.upload(s));
  OctView v{};
  char* di = st->run.dev_in(); char* dout = st->run.dev_out();
  v.lists = s_lists.in(di); v.xy = xy; v.response = response; v.work = st->work.as<unsigned short>();
  v.out_index = o_index.in(dout); v.out_count = o_count.in(dout); v.out_status = o_status.in(dout);
  hipLaunchKernelGGL(k_octree, dim3((unsigned)n_lists), dim3(kOctBlock), kOctLdsBytes, s, v);
  OSH_TRY(launch_check("octree"));
  OSH_HIP(hipMemcpyAsync(st->run.host_out(), dout, head_bytes, hipMemcpyDeviceToHost, s));
  OSH_HIP(hipStreamSynchronize(s));
  count.assign(o_count.in(st->run.host_out()), o_count.in(st->run.host_out()) + n_lists);
  status.assign(o_status.in(st->run.host_out()), o_status.in(st->run.host_out()) + n_lists);
  *index = o_index.in(dout);
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_octree_distribute(osh_orb_ctx* c, int32_t n_lists, const osh_octree_list* lists, osh_octree_result* results) {
  PhaseClock clock;
  if (n_lists < 0 || (n_lists && (!lists || !results))) { set_error("osh_orb_octree_distribute: bad arguments"); return OSH_ERR_INVALID; }
  size_t total = 0, total_out = 0;
  for (int k = 0; k < n_lists; ++k) {   // a refusal needs no context and no device
    const osh_octree_list& l = lists[k];
    const char* why = "";
    const int rc = oct_validate_list(l.n, l.xy, l.response, l.width, l.height, l.n_features, &why);
    if (rc != kOctOk) { set_error("osh_orb_octree_distribute: list %d: %s", k, why); return rc; }
    if (results[k].capacity < 0 || (results[k].capacity && !results[k].index)) { set_error("osh_orb_octree_distribute: list %d: bad result array", k); return OSH_ERR_INVALID; }
    total += (size_t)l.n; total_out += (size_t)std::min(l.n, kOctMaxNodes);
  }
  if (n_lists > (1 << 20) || total > (size_t)1 << 28) { set_error("osh_orb_octree_distribute: batch too large"); return OSH_ERR_UNSUPPORTED; }
  if (!c) { set_error("osh_orb_octree_distribute: no context"); return OSH_ERR_INVALID; }
  if (n_lists == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  OctreeState* st = orb_state<OctreeState>(c, kOrbAttachOctree);
  clock.profiling = orb_profiling(c);
  // the candidates up; the lists, the kernel and the counts are octree_run's
  Layout in, out;
  const auto s_xy = in.take<float2>(total);
  const auto s_resp = in.take<float>(total);
  out.take<int>(1);   // nothing comes back through this staging
  OSH_TRY(st->call.reserve(in, out));
  char* h = st->call.host_in();
  std::vector<OctListDev> dl((size_t)n_lists);
  size_t key0 = 0;
  for (int k = 0; k < n_lists; ++k) {
    const osh_octree_list& l = lists[k];
    dl[k] = {(int)key0, l.n, l.width, l.height, l.n_features, 0, 0};
    if (l.n) { std::memcpy(s_xy.in(h) + key0, l.xy, (size_t)l.n * 8); std::memcpy(s_resp.in(h) + key0, l.response, (size_t)l.n * 4); }
    key0 += (size_t)l.n;
  }
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));
  std::vector<int> count, status;
  const int* d_index = nullptr;
  OSH_TRY(octree_run(c, s, dl, s_xy.in(st->call.dev_in()), s_resp.in(st->call.dev_in()), count, status, &d_index));
  clock.mark();
  std::vector<int> kept(total_out);
  if (total_out) {
    OSH_HIP(hipMemcpyAsync(kept.data(), d_index, total_out * sizeof(int), hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
  }
  int rc = OSH_OK;
  for (int k = 0; k < n_lists; ++k) {
    osh_octree_result& r = results[k];
    r.status = status[k]; r.n_out = count[k];
    if (r.status != OSH_OK && rc == OSH_OK) { rc = r.status; set_error("osh_orb_octree_distribute: list %d reached a loop bound", k); }
    if (r.status != OSH_OK || r.n_out > r.capacity) continue;   // the count only: the caller sizes its array and calls again
    if (r.n_out) std::memcpy(r.index, kept.data() + dl[k].out0, (size_t)r.n_out * sizeof(int));
  }
  clock.mark();
  clock.store(st->ms);
  return rc;
}

extern "C" int osh_orb_octree_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<OctreeState>("osh_orb_octree_get_times", c, kOrbAttachOctree, ms);
}
