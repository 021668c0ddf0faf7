// keyframe_cull_device.hip -- the counts of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:932-1089) on MI355X (gfx950); the rule
// is that of keyframe_cull.h.
//
// osh_orb_keyframe_cull_stage packs the problem into three record arrays (a 16-byte point record, one word per observation, the
// slots) and keeps them on the device; osh_orb_keyframe_cull_count uploads a removed mask of 128 words, launches k_keyframe_cull_count
// once and downloads three integers per candidate.  A KeyFrameCulling call that culls n keyframes makes n + 1 count calls.
//
// k_keyframe_cull_count: one block of 1024 threads per candidate, the removed mask of the whole table in LDS (512 bytes).  A group of
// 16 lanes takes a slot: it reads the slot's point record once and walks the point's observation run 16 words at a time (one
// 64-byte segment per group), a loop, so a run of any length is handled.  Each lane classifies its observation (kc_observer); the
// group's sums come from three ballots and population counts over the group's 16 bits of the wave's mask: the observers that count,
// and bit 0 and bit 1 of the weights of the removed ones.  From those sums every lane of the group has n_obs', bad' and the slot's
// two verdict bits (kc_slot_verdict).  Seen from the slots of a candidate, the observation runs of the generator
// (synth_keyframe_cull.random_scene) have a median of 18 and a mean of 34; 46 % are at most 16 long, 79 % at most 32, and 9 % are
// longer than 64, so nearly every set of 64 slots holds one such run.  A lane per slot that walks its run alone would keep every wave
// for 65 or more dependent loads of 64 unrelated addresses with most lanes idle; so the lane group is the shape chosen, and 16 lanes
// (a median run in two steps, four slots per wave in flight) rather than 32, which would idle half its lanes on every second slot.
// The per-candidate sums are integer adds: across the four groups of a wave by two shuffles, across the 16 waves through LDS in
// wave order by one thread, which also takes the float32 decision (kc_decide).  No atomics; nothing depends on timing.
#include "common.h"
#include "keyframe_cull.h"
#include "orb_stage.h"
#include <chrono>
#include <vector>

namespace osh {

constexpr int kKcBlock = 1024;
constexpr int kKcWaves = kKcBlock / 64;
constexpr int kKcGroup = 16;                                 // lanes per slot
constexpr int kKcMaskWords = OSH_KFCULL_MAX_KEYFRAMES / 32;
static_assert(OSH_KFCULL_MAX_KEYFRAMES <= 65536, "kc_obs_word keeps the table index in 16 bits");
static_assert(kKcMaskWords <= kKcBlock, "one thread per mask word");

struct KcCount {
  KcView v;
  const uint32_t* mask;   // [kKcMaskWords]
  int first;              // blockIdx.x is candidate first + blockIdx.x
  float redundant_th;
  int* n_mps; int* n_redundant; int* redundant;   // [gridDim.x]
};

// grid = candidates evaluated
__global__ __launch_bounds__(kKcBlock) void k_keyframe_cull_count(KcCount d) {
  __shared__ uint32_t s_mask[kKcMaskWords];
  __shared__ int s_sum[2][kKcWaves];
  const int tid = (int)threadIdx.x;
  if (tid < kKcMaskWords) s_mask[tid] = d.mask[tid];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int group = lane / kKcGroup, sub = lane % kKcGroup, shift = group * kKcGroup;
  const int k = d.first + (int)blockIdx.x;
  const int s0 = d.v.cand_slot_off[k], s1 = d.v.cand_slot_off[k + 1];
  int mps = 0, red = 0;
  // the four slots of a wave start at `base`, the same in all its lanes: every lane of the wave runs every ballot
  for (int base = s0 + wave * (64 / kKcGroup); base < s1; base += kKcBlock / kKcGroup) {
    const int s = base + group;
    const bool have = s < s1;
    KcPoint p{0, 0, 0, 0};
    int level = 0;
    if (have) { p = d.v.point[d.v.slot_point[s]]; level = d.v.slot_level[s]; }
    int longest = max(p.count, __shfl_xor(p.count, 16));
    longest = max(longest, __shfl_xor(longest, 32));
    int lost = 0, others = 0;
    for (int e0 = 0; e0 < longest; e0 += kKcGroup) {
      const int e = e0 + sub;
      const bool in = e < p.count;
      const uint32_t w = in ? d.v.obs[(size_t)p.first + (size_t)e] : 0u;
      int l; bool c;
      kc_observer(w, s_mask, k, level, l, c);
      if (!in) { l = 0; c = false; }
      const unsigned long long b_c = __builtin_amdgcn_ballot_w64(c);
      const unsigned long long b_0 = __builtin_amdgcn_ballot_w64((l & 1) != 0), b_1 = __builtin_amdgcn_ballot_w64((l & 2) != 0);
      others += __popc((unsigned)(b_c >> shift) & 0xffffu);
      lost += __popc((unsigned)(b_0 >> shift) & 0xffffu) + 2 * __popc((unsigned)(b_1 >> shift) & 0xffffu);
    }
    int mp, r;
    kc_slot_verdict(p.n_obs, p.bad, lost, others, mp, r);
    if (have && sub == 0) { mps += mp; red += r; }
  }
  // lanes 0, 16, 32 and 48 hold the sums of their groups, the others zero
  mps += __shfl_xor(mps, 16); mps += __shfl_xor(mps, 32);
  red += __shfl_xor(red, 16); red += __shfl_xor(red, 32);
  if (lane == 0) { s_sum[0][wave] = mps; s_sum[1][wave] = red; }
  __syncthreads();
  if (tid == 0) {
    int a = 0, b = 0;
    for (int w = 0; w < kKcWaves; ++w) { a += s_sum[0][w]; b += s_sum[1][w]; }
    d.n_mps[blockIdx.x] = a; d.n_redundant[blockIdx.x] = b; d.redundant[blockIdx.x] = kc_decide(b, a, d.redundant_th);
  }
}

struct KfCullState {
  StagedCall problem;   // the staged records: [in] only
  StagedCall count;     // per count call: [in] the mask, [out] three integers per candidate
  bool staged = false;
  int n_keyframes = 0, n_candidates = 0;
  float redundant_th = 0.f;
  Section<int> s_off, s_slot_point, s_slot_level;
  Section<KcPoint> s_point;
  Section<uint32_t> s_obs;
  double ms[4] = {0, 0, 0, 0};
};

struct KcTotals { size_t slots = 0, points = 0, obs = 0; };

static int kc_validate(const osh_kfcull_problem& g, KcTotals* totals) {
  const char* me = "osh_orb_keyframe_cull_stage";
  if (g.n_keyframes < 0 || g.n_candidates < 0 || g.n_points < 0) { set_error("%s: negative count", me); return OSH_ERR_INVALID; }
  if (g.n_candidates > OSH_KFCULL_MAX_CANDIDATES) { set_error("%s: %d candidates, more than OSH_KFCULL_MAX_CANDIDATES = %d", me, g.n_candidates, OSH_KFCULL_MAX_CANDIDATES); return OSH_ERR_UNSUPPORTED; }
  if (g.n_keyframes > OSH_KFCULL_MAX_KEYFRAMES) { set_error("%s: %d keyframes, more than OSH_KFCULL_MAX_KEYFRAMES = %d", me, g.n_keyframes, OSH_KFCULL_MAX_KEYFRAMES); return OSH_ERR_UNSUPPORTED; }
  if (g.n_points > OSH_KFCULL_MAX_POINTS) { set_error("%s: %d points, more than OSH_KFCULL_MAX_POINTS = %d", me, g.n_points, OSH_KFCULL_MAX_POINTS); return OSH_ERR_UNSUPPORTED; }
  if (g.n_candidates > g.n_keyframes) { set_error("%s: %d candidates in a table of %d keyframes", me, g.n_candidates, g.n_keyframes); return OSH_ERR_INVALID; }
  if ((g.n_candidates && !g.cand_slot_off) || (g.n_points && (!g.point_obs_off || !g.point_n_obs || !g.point_bad))) { set_error("%s: NULL array", me); return OSH_ERR_INVALID; }
  KcTotals t;
  t.points = (size_t)g.n_points;
  const long n_slots = g.n_candidates ? (long)g.cand_slot_off[g.n_candidates] : 0, n_obs = g.n_points ? (long)g.point_obs_off[g.n_points] : 0;
  if (n_slots > OSH_KFCULL_MAX_SLOTS) { set_error("%s: %ld slots, more than OSH_KFCULL_MAX_SLOTS = %d", me, n_slots, OSH_KFCULL_MAX_SLOTS); return OSH_ERR_UNSUPPORTED; }
  if (n_obs > OSH_KFCULL_MAX_OBSERVATIONS) { set_error("%s: %ld observations, more than OSH_KFCULL_MAX_OBSERVATIONS = %d", me, n_obs, OSH_KFCULL_MAX_OBSERVATIONS); return OSH_ERR_UNSUPPORTED; }
  if (n_slots < 0 || n_obs < 0) { set_error("%s: negative total", me); return OSH_ERR_INVALID; }
  if (g.n_candidates && g.cand_slot_off[0] != 0) { set_error("%s: cand_slot_off[0] is %d, not 0", me, g.cand_slot_off[0]); return OSH_ERR_INVALID; }
  if (g.n_points && g.point_obs_off[0] != 0) { set_error("%s: point_obs_off[0] is %d, not 0", me, g.point_obs_off[0]); return OSH_ERR_INVALID; }
  for (int c = 0; c < g.n_candidates; ++c)
    if (g.cand_slot_off[c + 1] < g.cand_slot_off[c] || g.cand_slot_off[c + 1] > n_slots) { set_error("%s: candidate %d: cand_slot_off decreases or passes its last entry", me, c); return OSH_ERR_INVALID; }
  for (int p = 0; p < g.n_points; ++p) {
    if (g.point_obs_off[p + 1] < g.point_obs_off[p] || g.point_obs_off[p + 1] > n_obs) { set_error("%s: point %d: point_obs_off decreases or passes its last entry", me, p); return OSH_ERR_INVALID; }
    if (g.point_bad[p] > 1) { set_error("%s: point %d: point_bad is %d", me, p, (int)g.point_bad[p]); return OSH_ERR_INVALID; }
  }
  if (n_slots && (!g.slot_point || !g.slot_level)) { set_error("%s: NULL slot array with %ld slots", me, n_slots); return OSH_ERR_INVALID; }
  if (n_obs && (!g.obs_kf || !g.obs_level || !g.obs_weight)) { set_error("%s: NULL observation array with %ld observations", me, n_obs); return OSH_ERR_INVALID; }
  for (long s = 0; s < n_slots; ++s) {
    if (g.slot_point[s] < 0 || g.slot_point[s] >= g.n_points) { set_error("%s: slot %ld: point %d outside [0, %d)", me, s, g.slot_point[s], g.n_points); return OSH_ERR_INVALID; }
    if (g.slot_level[s] < 0 || g.slot_level[s] > 255) { set_error("%s: slot %ld: level %d outside [0, 255]", me, s, g.slot_level[s]); return OSH_ERR_INVALID; }
  }
  for (long e = 0; e < n_obs; ++e) {
    if (g.obs_kf[e] < 0 || g.obs_kf[e] >= g.n_keyframes) { set_error("%s: observation %ld: keyframe %d outside [0, %d)", me, e, g.obs_kf[e], g.n_keyframes); return OSH_ERR_INVALID; }
    if (g.obs_level[e] < 0 || g.obs_level[e] > 255) { set_error("%s: observation %ld: level %d outside [0, 255]", me, e, g.obs_level[e]); return OSH_ERR_INVALID; }
    if (g.obs_weight[e] < 1 || g.obs_weight[e] > 3) { set_error("%s: observation %ld: weight %d outside 1..3", me, e, g.obs_weight[e]); return OSH_ERR_INVALID; }
  }
  t.slots = (size_t)n_slots; t.obs = (size_t)n_obs;
  *totals = t;
  return OSH_OK;
}

using kc_clock = std::chrono::steady_clock;
static double kc_ms(kc_clock::time_point a, kc_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_keyframe_cull_stage(osh_orb_ctx* c, const osh_kfcull_problem* problem) {
  const auto t0 = kc_clock::now();
  if (!problem) { set_error("osh_orb_keyframe_cull_stage: bad arguments"); return OSH_ERR_INVALID; }
  KcTotals tot;
  OSH_TRY(kc_validate(*problem, &tot));   // the problem first: a refusal needs no context and no device
  if (!c) { set_error("osh_orb_keyframe_cull_stage: no context"); return OSH_ERR_INVALID; }
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  KfCullState* st = orb_state<KfCullState>(c, kOrbAttachKfCull);
  st->staged = false;
  const osh_kfcull_problem& g = *problem;

  Layout in, none;
  st->s_off = in.take<int>((size_t)g.n_candidates + 1);
  st->s_slot_point = in.take<int>(tot.slots); st->s_slot_level = in.take<int>(tot.slots);
  st->s_point = in.take<KcPoint>(tot.points);
  st->s_obs = in.take<uint32_t>(tot.obs);
  none.take<int>(0);   // a StagedCall wants an output buffer; an empty section still has one
  OSH_TRY(st->problem.reserve(in, none));
  char* h = st->problem.host_in();
  if (g.n_candidates) std::memcpy(st->s_off.in(h), g.cand_slot_off, ((size_t)g.n_candidates + 1) * 4); else st->s_off.in(h)[0] = 0;
  if (tot.slots) { std::memcpy(st->s_slot_point.in(h), g.slot_point, tot.slots * 4); std::memcpy(st->s_slot_level.in(h), g.slot_level, tot.slots * 4); }
  for (size_t p = 0; p < tot.points; ++p)
    st->s_point.in(h)[p] = KcPoint{g.point_obs_off[p], g.point_obs_off[p + 1] - g.point_obs_off[p], g.point_n_obs[p], (int)g.point_bad[p]};
  for (size_t e = 0; e < tot.obs; ++e) st->s_obs.in(h)[e] = kc_obs_word(g.obs_kf[e], g.obs_level[e], g.obs_weight[e]);
  const auto t1 = kc_clock::now();
  OSH_TRY(st->problem.upload(s));
  OSH_HIP(hipStreamSynchronize(s));   // the pinned copy is free for the next stage call
  const auto t2 = kc_clock::now();
  st->n_keyframes = g.n_keyframes; st->n_candidates = g.n_candidates; st->redundant_th = g.redundant_th;
  st->staged = true;
  if (orb_profiling(c)) { st->ms[0] = kc_ms(t0, t1); st->ms[1] = kc_ms(t1, t2); st->ms[2] = 0; st->ms[3] = 0; }
  return OSH_OK;
}

extern "C" int osh_orb_keyframe_cull_count(osh_orb_ctx* c, int32_t n_removed, const int32_t* removed_kf, int32_t first_candidate,
                                           const osh_kfcull_result* result) {
  const auto t0 = kc_clock::now();
  const char* me = "osh_orb_keyframe_cull_count";
  if (n_removed < 0 || (n_removed && !removed_kf) || !result) { set_error("%s: bad arguments", me); return OSH_ERR_INVALID; }
  if (first_candidate < 0 || first_candidate > OSH_KFCULL_MAX_CANDIDATES) { set_error("%s: first_candidate %d outside [0, %d]", me, first_candidate, OSH_KFCULL_MAX_CANDIDATES); return OSH_ERR_INVALID; }
  for (int i = 0; i < n_removed; ++i)
    if (removed_kf[i] < 0 || removed_kf[i] >= OSH_KFCULL_MAX_KEYFRAMES) { set_error("%s: removed keyframe %d outside [0, %d)", me, removed_kf[i], OSH_KFCULL_MAX_KEYFRAMES); return OSH_ERR_INVALID; }
  if (!c) { set_error("%s: no context", me); return OSH_ERR_INVALID; }
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  KfCullState* st = orb_state<KfCullState>(c, kOrbAttachKfCull);
  if (!st->staged) { set_error("%s: no staged problem", me); return OSH_ERR_INVALID; }
  if (first_candidate > st->n_candidates) { set_error("%s: first_candidate %d above the %d staged candidates", me, first_candidate, st->n_candidates); return OSH_ERR_INVALID; }
  for (int i = 0; i < n_removed; ++i)
    if (removed_kf[i] >= st->n_keyframes) { set_error("%s: removed keyframe %d outside the staged table of %d", me, removed_kf[i], st->n_keyframes); return OSH_ERR_INVALID; }
  const int n = st->n_candidates - first_candidate;
  if (n == 0) return OSH_OK;

  Layout in, out;
  const auto s_mask = in.take<uint32_t>(kKcMaskWords);
  const auto o_mps = out.take<int>(OSH_KFCULL_MAX_CANDIDATES), o_red = out.take<int>(OSH_KFCULL_MAX_CANDIDATES), o_dec = out.take<int>(OSH_KFCULL_MAX_CANDIDATES);
  OSH_TRY(st->count.reserve(in, out));
  uint32_t* mask = s_mask.in(st->count.host_in());
  std::memset(mask, 0, kKcMaskWords * 4);
  for (int i = 0; i < n_removed; ++i) mask[removed_kf[i] >> 5] |= 1u << (removed_kf[i] & 31);
  OSH_TRY(st->count.upload(s));
  char* dp = st->problem.dev_in();
  KcCount d{};
  d.v.cand_slot_off = st->s_off.in(dp); d.v.slot_point = st->s_slot_point.in(dp); d.v.slot_level = st->s_slot_level.in(dp);
  d.v.point = st->s_point.in(dp); d.v.obs = st->s_obs.in(dp);
  d.mask = s_mask.in(st->count.dev_in());
  d.first = first_candidate; d.redundant_th = st->redundant_th;
  char* dout = st->count.dev_out();
  d.n_mps = o_mps.in(dout); d.n_redundant = o_red.in(dout); d.redundant = o_dec.in(dout);
  hipLaunchKernelGGL(k_keyframe_cull_count, dim3((unsigned)n), dim3(kKcBlock), 0, s, d);
  OSH_TRY(launch_check("keyframe cull count"));
  const bool profiling = orb_profiling(c);
  if (profiling) OSH_HIP(hipStreamSynchronize(s));
  const auto t1 = kc_clock::now();
  OSH_TRY(st->count.download(s));
  const char* ho = st->count.host_out();
  if (result->n_mps) std::memcpy(result->n_mps, o_mps.in(ho), (size_t)n * 4);
  if (result->n_redundant) std::memcpy(result->n_redundant, o_red.in(ho), (size_t)n * 4);
  if (result->redundant) for (int i = 0; i < n; ++i) result->redundant[i] = (uint8_t)o_dec.in(ho)[i];
  if (profiling) { st->ms[2] = kc_ms(t0, t1); st->ms[3] = kc_ms(t1, kc_clock::now()); }
  return OSH_OK;
}

extern "C" int osh_orb_keyframe_cull_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<KfCullState>("osh_orb_keyframe_cull_get_times", c, kOrbAttachKfCull, ms);
}
