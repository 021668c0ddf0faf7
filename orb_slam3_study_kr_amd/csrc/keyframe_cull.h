// keyframe_cull.h -- the counting rule of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:932-1089), stated once for the
// host and for the kernel of keyframe_cull_device.hip.  Every quantity is an integer but the one float32 comparison of kc_decide.
//
// A call has a keyframe table (the candidates first, in list order, then every other observer), and three kinds of record:
//   observation  one per (point, observer keyframe): the observer's table index `kf`, its `level` (the reference's scaleLeveli,
//                :1013-1026: the left octave, lowered to the right one of a rig when that is smaller or the left is absent) and its
//                `weight`, what MapPoint::EraseObservation (src/MapPoint.cc:178-186) subtracts from nObs for it (1..3);
//   point        `n_obs` (the point's own nObs when the call was staged, not a sum), `bad`, and its run of observations;
//   slot         one per slot of a candidate that holds a point and passes the depth test of :989-993: the point and the slot's
//                `level` (scaleLevel, :1001-1003; a right slot i of a rig reads mvKeysRight[i - NLeft]).
// A removed set is a bit mask over the table.  The state of a point under a removed set,
//   n_obs' = n_obs - sum of the weights of its removed observers,   bad' = bad || (an observer is removed && n_obs' <= 2),
// is what the map holds after KeyFrame::SetBadFlag of every keyframe of the set, in any order: each EraseObservation subtracts its
// weight and tests nObs <= 2, nObs only falls, so the point is bad after the last of them exactly when the final value is <= 2.
// The verdict of candidate k counts, over its slots whose point is not bad', nMPs (all of them) and nRedundant (n_obs' > 3 and more
// than 3 observers that are neither removed nor k itself have level <= slot level + 1).  The reference leaves its walk over the
// observers at the fourth hit (:1031); that only shortens the walk, the count of hits is compared with 3 either way, so the order
// of its std::map (by pointer value) does not enter the result and the whole run may be counted in any order.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OSH_KC_HD __host__ __device__ inline
#else
#define OSH_KC_HD inline
#endif

namespace osh {

constexpr int kKcThObs = 3;   // thObs of :978-979

// One observation in a word: table index in bits 0-15, level in bits 16-23, weight in bits 24-25.
OSH_KC_HD uint32_t kc_obs_word(int kf, int level, int weight) { return (uint32_t)kf | ((uint32_t)level << 16) | ((uint32_t)weight << 24); }
OSH_KC_HD int kc_obs_kf(uint32_t w) { return (int)(w & 0xffffu); }
OSH_KC_HD int kc_obs_level(uint32_t w) { return (int)((w >> 16) & 0xffu); }
OSH_KC_HD int kc_obs_weight(uint32_t w) { return (int)((w >> 24) & 3u); }

OSH_KC_HD bool kc_removed(const uint32_t* mask, int kf) { return (mask[kf >> 5] >> (kf & 31)) & 1u; }

// What one observation adds for a slot of candidate k at `slot_level`: the weight it takes from n_obs (removed observers) and
// whether it is one of the "other observers at the same or a finer scale"
OSH_KC_HD void kc_observer(uint32_t w, const uint32_t* mask, int k, int slot_level, int& lost, bool& counts) {
  const int kf = kc_obs_kf(w);
  const bool gone = kc_removed(mask, kf);
  lost = gone ? kc_obs_weight(w) : 0;
  counts = !gone && kf != k && kc_obs_level(w) <= slot_level + 1;
}

// The slot's part of the verdict from the sums over its point's run: `lost`, the weights of the removed observers (every weight is
// at least 1, so lost > 0 says that an observer is removed), and `others`
OSH_KC_HD void kc_slot_verdict(int n_obs, int bad, int lost, int others, int& is_mp, int& is_redundant) {
  const int n = n_obs - lost;
  const bool bad_now = bad != 0 || (lost > 0 && n <= 2);
  is_mp = bad_now ? 0 : 1;
  is_redundant = (!bad_now && n > kKcThObs && others > kKcThObs) ? 1 : 0;
}

// :1044, nRedundantObservations > redundant_th * nMPs in float32, the product rounded before the comparison
OSH_KC_HD int kc_decide(int n_redundant, int n_mps, float redundant_th) {
#pragma clang fp contract(off)
  const float limit = redundant_th * (float)n_mps;
  return (float)n_redundant > limit ? 1 : 0;
}

// A point: its run of observations, its own nObs and whether it is bad, when the call was staged (one 16-byte load)
struct alignas(16) KcPoint { int first, count, n_obs, bad; };

// The arrays of a call (host or device memory)
struct KcView {
  const int* cand_slot_off;     // [n_candidates + 1]
  const int* slot_point;        // [n_slots]
  const int* slot_level;        // [n_slots]
  const KcPoint* point;         // [n_points]
  const uint32_t* obs;          // [n_obs] kc_obs_word
};

// Candidate k on one thread (the host build)
inline void kc_count_candidate(const KcView& v, const uint32_t* mask, int k, int& n_mps, int& n_redundant) {
  n_mps = 0; n_redundant = 0;
  for (int s = v.cand_slot_off[k]; s < v.cand_slot_off[k + 1]; ++s) {
    const KcPoint p = v.point[v.slot_point[s]];
    int lost = 0, others = 0;
    for (int e = p.first; e < p.first + p.count; ++e) {
      int l; bool c;
      kc_observer(v.obs[e], mask, k, v.slot_level[s], l, c);
      lost += l; others += c ? 1 : 0;
    }
    int mp, red;
    kc_slot_verdict(p.n_obs, p.bad, lost, others, mp, red);
    n_mps += mp; n_redundant += red;
  }
}

}  // namespace osh
