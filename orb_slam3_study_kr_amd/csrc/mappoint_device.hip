// mappoint_device.hip -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403) and MapPoint::UpdateNormalAndDepth
// (:426-494) on MI355X (gfx950) for batches of map points; the statements are those of mappoint_refresh.h.
//
// A call is about a thousand independent problems of 2-60 entries with a long tail, so the points are sorted into two classes when
// the call is packed and each class has its kernel:
//   k_mappoint_wave   a wavefront per point of at most 64 entries, four points per block.  Lane j holds descriptor j; row i is read
//                     from the wave's LDS copy (one address for all lanes: a broadcast); lane j computes d(i, j).
//   k_mappoint_block  a block per point of 65..OSH_MAPPOINT_MAX_DESCRIPTORS entries.  The descriptors are in LDS, every wave holds
//                     all of them in registers (four per lane), and the waves share the rows.
// The median of a row is not sorted out: the element of rank (M - 1) / 2 is fixed bit by bit from the top of the 9-bit distance,
// each bit by one ballot and one population count per 64 distances (mp_select).  All lanes of a wave follow the same rows in
// ascending order, so "the first row with the least median" needs no exchange inside a wave; the block class takes the minimum of
// (median << 16 | row) over its four waves through LDS.  The unit vectors of the entries are independent (one per lane); their
// sum is one chain in entry order.  No atomics: every point's seven result words are written by one lane.
#include "common.h"
#include "mappoint_refresh.h"
#include "orb_hamming.h"
#include "orb_stage.h"
#include <vector>

namespace osh {

constexpr int kMpBlock = 256;
constexpr int kMpWaves = kMpBlock / 64;                     // points per block of the wavefront class
constexpr int kMpMax = OSH_MAPPOINT_MAX_DESCRIPTORS;
constexpr int kMpSlices = kMpMax / 64;                      // descriptors a lane holds in the block class
static_assert(kMpMax % 64 == 0 && kMpMax <= kMpBlock, "k_mappoint_block loads one entry per thread");

struct MpView {
  const MpPoint* point;      // [P] in the order of the call
  const int* order;          // [P] the points of the wavefront class, then those of the block class
  const uint4* desc;         // two per entry
  const int* centre;         // index into centres, over all batches
  const unsigned char* use;
  const float* centres;
  int* best_entry; int* best_median; float* normal; float* min_distance; float* max_distance;
  int n_wave, n_block;
};

// The element of rank `rank` (from 0) among the distances d[t] of the lanes with valid[t], all lanes of the wave together.
template <int T>
__device__ __forceinline__ int mp_select(const unsigned (&d)[T], const bool (&valid)[T], int rank) {
  bool in[T];
#pragma unroll
  for (int t = 0; t < T; ++t) in[t] = valid[t];
  unsigned value = 0;
#pragma unroll
  for (int bit = 8; bit >= 0; --bit) {
    int zeros = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) zeros += __popcll(__builtin_amdgcn_ballot_w64(in[t] && !((d[t] >> bit) & 1u)));
    const bool one = rank >= zeros;   // the same in every lane
    if (one) { rank -= zeros; value |= 1u << bit; }
#pragma unroll
    for (int t = 0; t < T; ++t) in[t] = in[t] && (((d[t] >> bit) & 1u) != 0) == one;
  }
  return (int)value;
}

__device__ __forceinline__ void mp_write(const MpView& v, int pid, const MpOut& o) {
  v.best_entry[pid] = o.best_entry; v.best_median[pid] = o.best_median;
  v.normal[3 * (size_t)pid] = o.normal[0]; v.normal[3 * (size_t)pid + 1] = o.normal[1]; v.normal[3 * (size_t)pid + 2] = o.normal[2];
  v.min_distance[pid] = o.min_distance; v.max_distance[pid] = o.max_distance;
}

// grid = ceil(n_wave / 4)
__global__ __launch_bounds__(kMpBlock) void k_mappoint_wave(MpView v) {
#pragma clang fp contract(off)
  __shared__ uint4 s_desc[kMpWaves][64 * 2];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int slot = (int)blockIdx.x * kMpWaves + wave;
  const bool have = slot < v.n_wave;
  int pid = 0;
  MpPoint p{};
  if (have) { pid = v.order[slot]; p = v.point[pid]; }
  const int n = p.n;   // 0 without a point
  uint4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
  bool valid = false;
  float u[3] = {0.f, 0.f, 0.f};
  if (lane < n) {
    const size_t e = (size_t)p.entry_base + (size_t)lane;
    a0 = v.desc[2 * e]; a1 = v.desc[2 * e + 1];
    valid = v.use[e] != 0;
    mp_unit_vector(p.pos, v.centres + 3 * (size_t)v.centre[e], u);
    s_desc[wave][2 * lane] = a0; s_desc[wave][2 * lane + 1] = a1;
  }
  __syncthreads();
  if (!have) return;
  MpOut o;
  if (n == 0) {
    mp_empty(o);
  } else {
    unsigned long long rows = __builtin_amdgcn_ballot_w64(valid);
    const int M = __popcll(rows), rank = mp_median_index(M);
    int best = 0x7fffffff, best_row = -1;
    while (rows) {
      const int i = __builtin_ctzll(rows);
      rows &= rows - 1;
      const unsigned d[1] = {hamming256(a0, a1, s_desc[wave][2 * i], s_desc[wave][2 * i + 1])};
      const bool in[1] = {valid};
      const int median = mp_select<1>(d, in, rank);
      if (median < best) { best = median; best_row = i; }
    }
    o.best_entry = best_row; o.best_median = M ? best : -1;
    float sum[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < n; ++j) {   // one chain in entry order; every lane runs it
      sum[0] = sum[0] + __shfl(u[0], j); sum[1] = sum[1] + __shfl(u[1], j); sum[2] = sum[2] + __shfl(u[2], j);
    }
    mp_finish(p, sum, v.centres + 3 * (size_t)p.ref_centre, o);
  }
  if (lane == 0) mp_write(v, pid, o);
}

// grid = n_block
__global__ __launch_bounds__(kMpBlock) void k_mappoint_block(MpView v) {
#pragma clang fp contract(off)
  __shared__ uint4 s_desc[kMpMax * 2];
  __shared__ float s_unit[kMpMax * 3];
  __shared__ unsigned char s_use[kMpMax];
  __shared__ float s_sum[3];
  __shared__ int s_best[kMpWaves];
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int pid = v.order[v.n_wave + (int)blockIdx.x];
  const MpPoint p = v.point[pid];
  const int n = p.n;   // 64 < n <= kMpMax
  if (tid < n) {
    const size_t e = (size_t)p.entry_base + (size_t)tid;
    s_desc[2 * tid] = v.desc[2 * e]; s_desc[2 * tid + 1] = v.desc[2 * e + 1];
    s_use[tid] = v.use[e];
    float u[3];
    mp_unit_vector(p.pos, v.centres + 3 * (size_t)v.centre[e], u);
    s_unit[3 * tid] = u[0]; s_unit[3 * tid + 1] = u[1]; s_unit[3 * tid + 2] = u[2];
  }
  __syncthreads();
  if (tid < 3) {   // one chain per component in entry order
    float s = 0.f;
    for (int j = 0; j < n; ++j) s = s + s_unit[3 * j + tid];
    s_sum[tid] = s;
  }
  uint4 a0[kMpSlices], a1[kMpSlices];
  bool valid[kMpSlices];
  int M = 0;
#pragma unroll
  for (int t = 0; t < kMpSlices; ++t) {
    const int j = lane + 64 * t;
    const bool inside = j < n;
    valid[t] = inside && s_use[inside ? j : 0] != 0;
    a0[t] = s_desc[inside ? 2 * j : 0]; a1[t] = s_desc[inside ? 2 * j + 1 : 1];
    M += __popcll(__builtin_amdgcn_ballot_w64(valid[t]));
  }
  const int rank = mp_median_index(M);
  int best = 0x7fffffff;   // (median << 16) | row
  for (int i = wave; i < n; i += kMpWaves) {
    if (!s_use[i]) continue;
    const uint4 b0 = s_desc[2 * i], b1 = s_desc[2 * i + 1];
    unsigned d[kMpSlices];
#pragma unroll
    for (int t = 0; t < kMpSlices; ++t) d[t] = hamming256(a0[t], a1[t], b0, b1);
    best = min(best, (mp_select<kMpSlices>(d, valid, rank) << 16) | i);
  }
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kMpWaves; ++w) best = min(best, s_best[w]);
    MpOut o;
    o.best_entry = M ? (best & 0xffff) : -1; o.best_median = M ? (best >> 16) : -1;
    const float sum[3] = {s_sum[0], s_sum[1], s_sum[2]};
    mp_finish(p, sum, v.centres + 3 * (size_t)p.ref_centre, o);
    mp_write(v, pid, o);
  }
}

struct MapPointState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
};

// Sizes of a call: points, entries and centres of all batches together
struct MpTotals { size_t points = 0, entries = 0, centres = 0; };

static int mp_validate(int n_batches, const osh_mappoint_batch* batches, MpTotals* totals) {
  MpTotals t;
  for (int b = 0; b < n_batches; ++b) {
    const osh_mappoint_batch& g = batches[b];
    if (g.n_points < 0 || g.n_centres < 0) { set_error("batch %d: negative count", b); return OSH_ERR_INVALID; }
    if (g.n_centres && !g.centres) { set_error("batch %d: NULL centres with n_centres = %d", b, g.n_centres); return OSH_ERR_INVALID; }
    t.centres += (size_t)g.n_centres;
    if (t.centres > (size_t)OSH_MAPPOINT_MAX_ENTRIES) { set_error("osh_orb_refresh_map_points: more than %d centres in one call", OSH_MAPPOINT_MAX_ENTRIES); return OSH_ERR_UNSUPPORTED; }
    if (g.n_points == 0) continue;
    if (!g.entry_off || !g.pos || !g.ref_centre || !g.level_scale || !g.top_scale) { set_error("batch %d: NULL point array with n_points = %d", b, g.n_points); return OSH_ERR_INVALID; }
    if (g.entry_off[0] != 0) { set_error("batch %d: entry_off[0] is %d, not 0", b, g.entry_off[0]); return OSH_ERR_INVALID; }
    const int n_entries = g.entry_off[g.n_points];
    if (n_entries > 0 && (!g.desc || !g.centre || !g.use_desc)) { set_error("batch %d: NULL entry array with %d entries", b, n_entries); return OSH_ERR_INVALID; }
    for (int p = 0; p < g.n_points; ++p) {
      const long count = (long)g.entry_off[p + 1] - (long)g.entry_off[p];
      if (count < 0) { set_error("batch %d: point %d: entry_off decreases", b, p); return OSH_ERR_INVALID; }
      if (count > OSH_MAPPOINT_MAX_DESCRIPTORS) {
        set_error("batch %d: point %d has %ld entries, more than OSH_MAPPOINT_MAX_DESCRIPTORS = %d", b, p, count, OSH_MAPPOINT_MAX_DESCRIPTORS);
        return OSH_ERR_INVALID;
      }
      if (count == 0) continue;
      if (g.ref_centre[p] < 0 || g.ref_centre[p] >= g.n_centres) { set_error("batch %d: point %d: ref_centre %d outside [0, %d)", b, p, g.ref_centre[p], g.n_centres); return OSH_ERR_INVALID; }
      for (int e = g.entry_off[p]; e < g.entry_off[p + 1]; ++e)
        if (g.centre[e] < 0 || g.centre[e] >= g.n_centres) {
          set_error("batch %d: point %d: entry %d: centre index %d outside [0, %d)", b, p, e - g.entry_off[p], g.centre[e], g.n_centres);
          return OSH_ERR_INVALID;
        }
    }
    t.points += (size_t)g.n_points; t.entries += (size_t)n_entries;
    if (t.points > (size_t)OSH_MAPPOINT_MAX_POINTS || t.entries > (size_t)OSH_MAPPOINT_MAX_ENTRIES) {
      set_error("osh_orb_refresh_map_points: more than %d points or %d entries in one call", OSH_MAPPOINT_MAX_POINTS, OSH_MAPPOINT_MAX_ENTRIES);
      return OSH_ERR_UNSUPPORTED;
    }
  }
  *totals = t;
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_refresh_map_points(osh_orb_ctx* c, int32_t n_batches, const osh_mappoint_batch* batches, const osh_mappoint_result* results) {
  PhaseClock clock;
  if (n_batches < 0 || (n_batches && (!batches || !results))) { set_error("osh_orb_refresh_map_points: bad arguments"); return OSH_ERR_INVALID; }
  MpTotals tot;
  OSH_TRY(mp_validate(n_batches, batches, &tot));   // the batches first: a refusal needs no context and no device
  if (!c) { set_error("osh_orb_refresh_map_points: no context"); return OSH_ERR_INVALID; }
  if (tot.points == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  MapPointState* st = orb_state<MapPointState>(c, kOrbAttachMapPoint);
  clock.profiling = orb_profiling(c);

  const size_t P = tot.points, E = tot.entries;
  Layout in, out;
  const auto s_point = in.take<MpPoint>(P);
  const auto s_order = in.take<int>(P);
  const auto s_desc = in.take<uint4>(E * 2);
  const auto s_centre = in.take<int>(E);
  const auto s_use = in.take<unsigned char>(E);
  const auto s_centres = in.take<float>(tot.centres * 3);
  const auto o_entry = out.take<int>(P); const auto o_median = out.take<int>(P);
  const auto o_normal = out.take<float>(P * 3); const auto o_min = out.take<float>(P); const auto o_max = out.take<float>(P);
  OSH_TRY(st->call.reserve(in, out));

  char* h = st->call.host_in();
  std::vector<size_t> base((size_t)n_batches);
  std::vector<int> big;
  size_t pb = 0, eb = 0, cb = 0;
  int n_wave = 0;
  for (int b = 0; b < n_batches; ++b) {
    const osh_mappoint_batch& g = batches[b];
    base[b] = pb;
    if (g.n_centres) std::memcpy(s_centres.in(h) + 3 * cb, g.centres, (size_t)g.n_centres * 12);
    const size_t ne = g.n_points ? (size_t)g.entry_off[g.n_points] : 0;
    if (ne) {
      std::memcpy(s_desc.in(h) + 2 * eb, g.desc, ne * 32);
      std::memcpy(s_use.in(h) + eb, g.use_desc, ne);
      for (size_t e = 0; e < ne; ++e) s_centre.in(h)[eb + e] = g.centre[e] + (int)cb;
    }
    for (int p = 0; p < g.n_points; ++p) {
      MpPoint& q = s_point.in(h)[pb + p];
      q.entry_base = (int)eb + g.entry_off[p]; q.n = g.entry_off[p + 1] - g.entry_off[p];
      q.pos[0] = g.pos[3 * (size_t)p]; q.pos[1] = g.pos[3 * (size_t)p + 1]; q.pos[2] = g.pos[3 * (size_t)p + 2];
      q.ref_centre = q.n ? g.ref_centre[p] + (int)cb : 0;
      q.level_scale = g.level_scale[p]; q.top_scale = g.top_scale[p];
      if (q.n <= 64) s_order.in(h)[n_wave++] = (int)(pb + p); else big.push_back((int)(pb + p));
    }
    pb += (size_t)g.n_points; eb += ne; cb += (size_t)g.n_centres;
  }
  const int n_block = (int)big.size();
  if (n_block) std::memcpy(s_order.in(h) + n_wave, big.data(), big.size() * sizeof(int));
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  MpView v{};
  v.point = s_point.in(di); v.order = s_order.in(di); v.desc = s_desc.in(di); v.centre = s_centre.in(di); v.use = s_use.in(di);
  v.centres = s_centres.in(di);
  v.best_entry = o_entry.in(dout); v.best_median = o_median.in(dout); v.normal = o_normal.in(dout);
  v.min_distance = o_min.in(dout); v.max_distance = o_max.in(dout);
  v.n_wave = n_wave; v.n_block = n_block;
  if (n_wave) {
    hipLaunchKernelGGL(k_mappoint_wave, dim3((unsigned)((n_wave + kMpWaves - 1) / kMpWaves)), dim3(kMpBlock), 0, s, v);
    OSH_TRY(launch_check("map point refresh (wavefront class)"));
  }
  if (n_block) {
    hipLaunchKernelGGL(k_mappoint_block, dim3((unsigned)n_block), dim3(kMpBlock), 0, s, v);
    OSH_TRY(launch_check("map point refresh (block class)"));
  }
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int b = 0; b < n_batches; ++b) {
    const osh_mappoint_result& r = results[b];
    const size_t n = (size_t)batches[b].n_points;
    scatter(r.best_entry, o_entry, ho, base[b], n); scatter(r.best_median, o_median, ho, base[b], n);
    scatter(r.normal, o_normal, ho, base[b], n, 3);
    scatter(r.min_distance, o_min, ho, base[b], n); scatter(r.max_distance, o_max, ho, base[b], n);
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_refresh_map_points_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<MapPointState>("osh_orb_refresh_map_points_get_times", c, kOrbAttachMapPoint, ms);
}
