// keyframe_cull_check.cpp -- csrc/keyframe_cull.h and PackKeyFrameCull (csrc/host/host_pack.h) as plain C++ under AddressSanitizer
// and UBSan: a program of its own (make keyframe-cull-check) that makes no HIP call and needs no device.  It runs the host build of
// the counting rule over the shapes of the generator (candidates of 0, 1, 63, 64, 65 and 257 slots, observation runs of 1, 16, 17, 70
// and 300, a table of OSH_KFCULL_MAX_KEYFRAMES entries with the last one removed, a mask of exactly the words the table needs) on
// exactly-sized arrays, so a read past an end is an AddressSanitizer report, and compares every count with a recount on a copy
// of the map from which the removed observers are really erased.  Then it packs small stand-in maps (no rig, a rig with left,
// right and both indices, a point in two slots, a bad candidate, a repeated candidate, far and negative depths) and checks the
// records by hand.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <vector>

#include "../../../include/orbslam3_hip.h"
#include "../keyframe_cull.h"
#include "host_pack.h"

using namespace ORB_SLAM3;

static long checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::fprintf(stderr, "keyframe_cull_check: line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

namespace {

struct Obs { int kf, level, weight; };
struct Point { int n_obs, bad; std::vector<Obs> obs; };
struct Slot { int point, level; };

struct Problem {
  int n_keyframes = 0;
  std::vector<Point> points;
  std::vector<std::vector<Slot>> cands;

  // the header's records, every array exactly as long as its content
  void count(const std::vector<int>& removed, std::vector<int>& n_mps, std::vector<int>& n_red) const {
    std::vector<int> off{0}, slot_point, slot_level;
    for (const auto& c : cands) { for (const Slot& s : c) { slot_point.push_back(s.point); slot_level.push_back(s.level); } off.push_back((int)slot_point.size()); }
    std::vector<osh::KcPoint> point;
    std::vector<uint32_t> obs;
    for (const Point& p : points) {
      point.push_back(osh::KcPoint{(int)obs.size(), (int)p.obs.size(), p.n_obs, p.bad});
      for (const Obs& o : p.obs) obs.push_back(osh::kc_obs_word(o.kf, o.level, o.weight));
    }
    std::vector<uint32_t> mask((size_t)(n_keyframes + 31) / 32, 0u);
    for (int k : removed) mask[k >> 5] |= 1u << (k & 31);
    const osh::KcView v{off.data(), slot_point.data(), slot_level.data(), point.data(), obs.data()};
    n_mps.assign(cands.size(), 0); n_red.assign(cands.size(), 0);
    for (size_t k = 0; k < cands.size(); ++k) osh::kc_count_candidate(v, mask.data(), (int)k, n_mps[k], n_red[k]);
  }
  // the definition: erase, then count from scratch
  void recount(const std::vector<int>& removed, std::vector<int>& n_mps, std::vector<int>& n_red) const {
    std::vector<Point> live = points;
    for (int k : removed)
      for (Point& p : live)
        for (size_t i = 0; i < p.obs.size(); ++i)
          if (p.obs[i].kf == k) { p.n_obs -= p.obs[i].weight; p.obs.erase(p.obs.begin() + i); if (p.n_obs <= 2) p.bad = 1; break; }
    n_mps.assign(cands.size(), 0); n_red.assign(cands.size(), 0);
    for (size_t k = 0; k < cands.size(); ++k)
      for (const Slot& s : cands[k]) {
        const Point& p = live[s.point];
        if (p.bad) continue;
        ++n_mps[k];
        if (p.n_obs <= 3) continue;
        int n = 0;
        for (const Obs& o : p.obs) if (o.kf != (int)k && o.level <= s.level + 1) ++n;
        if (n > 3) ++n_red[k];
      }
  }
  void check(const std::vector<int>& removed) const {
    std::vector<int> a, b, c, d;
    count(removed, a, b);
    recount(removed, c, d);
    CHECK(a == c && b == d);
  }
};

uint32_t rnd_state = 12345u;
int rnd(int n) { rnd_state = rnd_state * 1664525u + 1013904223u; return (int)((rnd_state >> 8) % (uint32_t)n); }

Problem shapes(int n_keyframes) {
  Problem pb;
  pb.n_keyframes = n_keyframes;
  for (int run : {1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 70, 300, 8, 8, 8, 8, 11, 11}) {
    Point p{0, rnd(20) == 0, {}};
    std::vector<char> used(n_keyframes, 0);
    for (int i = 0; i < run; ++i) {
      int k = (i == 0 && run > 8) ? n_keyframes - 1 : rnd(n_keyframes);   // the long runs hold the table's last entry
      while (used[k]) k = (k + 1) % n_keyframes;
      used[k] = 1;
      const Obs o{k, rnd(8), 1 + rnd(3)};
      p.obs.push_back(o);
      p.n_obs += o.weight;
    }
    p.n_obs += rnd(3) - 1;   // the point's own nObs need not be the sum
    pb.points.push_back(p);
  }
  for (int n : {0, 1, 63, 64, 65, 257}) {
    std::vector<Slot> c;
    for (int i = 0; i < n; ++i) c.push_back(Slot{rnd((int)pb.points.size()), rnd(8)});
    pb.cands.push_back(c);
  }
  return pb;
}

// ---- stand-in maps for the packer: members set directly, no method of the stand-ins' own bodies is needed
struct World {
  Map map;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> mps;
  GeometricCamera* cam2 = reinterpret_cast<GeometricCamera*>(&map);   // only ever compared with null

  KeyFrame* kf(unsigned long id, int n, int n_left) {
    kfs.emplace_back(new KeyFrame(id, &map));
    KeyFrame* k = kfs.back().get();
    k->N = n; k->NLeft = n_left; k->mThDepth = 40.f;
    k->mvpMapPoints.assign(n, nullptr); k->mvuRight.assign(n, -1.f); k->mvDepth.assign(n, 1.f);
    const int n_first = n_left == -1 ? n : n_left;
    k->mvKeysUn.assign(n_first, cv::KeyPoint()); k->mvKeys.assign(n_first, cv::KeyPoint()); k->mvKeysRight.assign(n - n_first, cv::KeyPoint());
    if (n_left != -1) k->mpCamera2 = cam2;
    return k;
  }
  MapPoint* mp() { mps.emplace_back(new MapPoint(mps.size(), Eigen::Vector3f(0.f, 0.f, 1.f), &map)); return mps.back().get(); }
  void see(KeyFrame* k, int slot, MapPoint* p, int octave) {   // src/MapPoint.cc:140-165
    k->mvpMapPoints[slot] = p;
    std::tuple<int, int>& idx = p->mObservations.emplace(k, std::tuple<int, int>(-1, -1)).first->second;
    if (k->NLeft != -1 && slot >= k->NLeft) { std::get<1>(idx) = slot; k->mvKeysRight[slot - k->NLeft].octave = octave; p->nObs += 1; }
    else { std::get<0>(idx) = slot; k->mvKeysUn[slot].octave = octave; k->mvKeys[slot].octave = octave; p->nObs += (!k->mpCamera2 && k->mvuRight[slot] >= 0) ? 2 : 1; }
  }
};

void pack_checks() {
  {   // no rig: stereo weights, the depth test, a point in two slots, a bad point kept, an empty slot
    World w;
    KeyFrame* a = w.kf(100, 6, -1);
    KeyFrame* o1 = w.kf(101, 2, -1);
    KeyFrame* o2 = w.kf(102, 2, -1);
    MapPoint *p = w.mp(), *q = w.mp(), *far = w.mp(), *neg = w.mp();
    a->mvuRight[0] = 5.f; o1->mvuRight[0] = 7.f;
    w.see(a, 0, p, 2); w.see(a, 1, q, 1); w.see(a, 3, p, 4);   // p twice: the later slot is its left index
    w.see(a, 4, far, 0); w.see(a, 5, neg, 0);
    a->mvDepth[4] = 40.5f; a->mvDepth[5] = -1.f;
    w.see(o1, 0, p, 3); w.see(o2, 1, p, 5); w.see(o2, 0, q, 0);
    q->mbBad = true;
    for (bool mono : {false, true}) {
      KeyFrameCullPack pk;
      PackKeyFrameCull({a}, mono, pk);
      const size_t slots = mono ? 5 : 3;
      CHECK(pk.n_candidates == 1 && pk.cand_slot_off.size() == 2 && pk.cand_slot_off[1] == (int)slots && pk.slot_point.size() == slots);
      CHECK(pk.points.size() == (mono ? 4u : 2u) && pk.points[0] == p && pk.points[1] == q);
      CHECK(pk.slot_index[0] == 0 && pk.slot_index[1] == 1 && pk.slot_index[2] == 3 && pk.slot_point[0] == 0 && pk.slot_point[2] == 0);
      CHECK(pk.slot_level[0] == 2 && pk.slot_level[1] == 1 && pk.slot_level[2] == 4);
      CHECK(pk.point_bad[0] == 0 && pk.point_bad[1] == 1);
      CHECK(pk.point_n_obs[0] == 2 + 1 + 2 + 1);   // a's slot 0 (stereo), a's slot 3, o1 (stereo), o2
      CHECK(pk.table.size() == 3 && pk.table[0] == a);
      CHECK(pk.point_obs_off[1] == 3 && pk.point_obs_off[2] == 5);
      for (int e = 0; e < 3; ++e) {
        KeyFrame* k = pk.table[pk.obs_kf[e]];
        CHECK(pk.obs_level[e] == (k == a ? 4 : k == o1 ? 3 : 5) && pk.obs_weight[e] == (k == o1 ? 2 : 1));   // a's left index is slot 3: no uRight
      }
      CHECK(pk.within_device_limits());
    }
  }
  {   // a rig: NLeft = 2, right slots 2 and 3
    World w;
    KeyFrame* a = w.kf(100, 4, 2);
    KeyFrame* both = w.kf(101, 4, 2);
    KeyFrame* right = w.kf(102, 4, 2);
    KeyFrame* plain = w.kf(103, 4, 2);
    plain->mpCamera2 = nullptr; plain->mvuRight[1] = 3.f;   // the left-stereo rule on: 2 for the left index, 1 more for the right
    MapPoint *p = w.mp(), *q = w.mp();
    w.see(a, 1, p, 3); w.see(a, 3, q, 6);                     // q in a right slot: its level is mvKeysRight[3 - 2]
    w.see(both, 0, p, 5); w.see(both, 2, p, 2);               // the right level is lower
    w.see(right, 3, p, 4);
    w.see(plain, 1, p, 1); w.see(plain, 3, p, 7);             // the left level is lower
    KeyFrameCullPack pk;
    PackKeyFrameCull({a}, true, pk);
    CHECK(pk.slot_point.size() == 2 && pk.slot_level[0] == 3 && pk.slot_level[1] == 6 && pk.slot_index[1] == 3);
    CHECK(pk.point_obs_off[1] == 4 && pk.point_obs_off[2] == 5);
    for (int e = 0; e < 4; ++e) {
      KeyFrame* k = pk.table[pk.obs_kf[e]];
      const int level = k == a ? 3 : k == both ? 2 : k == right ? 4 : 1, weight = k == a ? 1 : k == both ? 2 : k == right ? 1 : 3;
      CHECK(pk.obs_level[e] == level && pk.obs_weight[e] == weight);
    }
    CHECK(pk.point_n_obs[0] == 1 + 2 + 1 + 3);
  }
  {   // the list: a bad candidate, the map's initial keyframe and a repeated candidate keep their entries and get no slots
    World w;
    w.map.mnInitKFid = 7;
    KeyFrame* a = w.kf(100, 1, -1);
    KeyFrame* bad = w.kf(101, 1, -1);
    KeyFrame* init = w.kf(7, 1, -1);
    KeyFrame* other = w.kf(300, 1, -1);
    MapPoint* p = w.mp();
    w.see(a, 0, p, 0); w.see(bad, 0, p, 0); w.see(init, 0, p, 0); w.see(other, 0, p, 0);
    bad->mbBad = true;
    KeyFrameCullPack pk;
    PackKeyFrameCull({bad, a, init, a}, true, pk);
    CHECK(pk.n_candidates == 4 && pk.cand_slot_off.size() == 5);
    CHECK(pk.cand_slot_off[1] == 0 && pk.cand_slot_off[2] == 1 && pk.cand_slot_off[3] == 1 && pk.cand_slot_off[4] == 1);
    CHECK(pk.table.size() == 5 && pk.table[4] == other && pk.points.size() == 1 && pk.obs_kf.size() == 4);
    bool a_is_1 = false;
    for (int k : pk.obs_kf) a_is_1 = a_is_1 || k == 1;
    CHECK(a_is_1);   // the first occurrence of `a` is its table entry
    // the packed records through the rule: `a` has 3 other observers, not more than 3
    std::vector<osh::KcPoint> point{osh::KcPoint{0, 4, pk.point_n_obs[0], 0}};
    std::vector<uint32_t> obs;
    for (size_t e = 0; e < 4; ++e) obs.push_back(osh::kc_obs_word(pk.obs_kf[e], pk.obs_level[e], pk.obs_weight[e]));
    const std::vector<uint32_t> mask(1, 0u);
    const osh::KcView v{pk.cand_slot_off.data(), pk.slot_point.data(), pk.slot_level.data(), point.data(), obs.data()};
    int n_mps, n_red;
    osh::kc_count_candidate(v, mask.data(), 1, n_mps, n_red);
    CHECK(n_mps == 1 && n_red == 0 && osh::kc_decide(n_red, n_mps, 0.9f) == 0);
  }
}

}  // namespace

int main() {
  for (int n_keyframes : {301, 1000, OSH_KFCULL_MAX_KEYFRAMES}) {
    const Problem pb = shapes(n_keyframes);
    pb.check({});
    pb.check({0});
    pb.check({n_keyframes - 1});
    pb.check({64, 65, n_keyframes - 1, 5});
    std::vector<int> many;
    for (int i = 0; i < 60; ++i) { const int k = rnd(n_keyframes); bool dup = false; for (int m : many) dup = dup || m == k; if (!dup) many.push_back(k); }
    pb.check(many);
    for (const Point& p : pb.points) if (p.obs.size() > 8) pb.check({p.obs[0].kf, p.obs[1].kf, p.obs[2].kf});   // the observers of one point
  }
  // the float32 decision on both sides of its limits
  CHECK(osh::kc_decide(9, 10, 0.9f) == 0 && osh::kc_decide(10, 10, 0.9f) == 1 && osh::kc_decide(2, 4, 0.5f) == 0 && osh::kc_decide(3, 4, 0.5f) == 1);
  CHECK(osh::kc_decide(0, 0, 0.9f) == 0 && osh::kc_decide(0, 0, 0.5f) == 0);
  // the extremes of a word
  const uint32_t w = osh::kc_obs_word(OSH_KFCULL_MAX_KEYFRAMES - 1, 255, 3);
  CHECK(osh::kc_obs_kf(w) == OSH_KFCULL_MAX_KEYFRAMES - 1 && osh::kc_obs_level(w) == 255 && osh::kc_obs_weight(w) == 3);
  pack_checks();
  std::printf("keyframe_cull_check ok: %ld checks\n", checks);
  return 0;
}
