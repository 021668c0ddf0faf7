// orb_octree.h -- ORBextractor::DistributeOctTree (src/ORBextractor.cc:480-779) restated from the definition in
// include/orbslam3_hip.h: the quadtree that thins the FAST candidates of a pyramid level to about N keypoints.  Device code of
// orb_octree_device.hip; plain C++ as well, so the test library, ORBextractor::DistributeOctTreeDevice's fallback and
// `make octree-check` run the same statements on the host.
//
// The rule is integer and comparison only.  The reference keeps a std::list of nodes and pushes children to its front; here a list
// is an array in front-to-back order that every round rebuilds, because where a node lands is a function of counts alone:
//   * a round walks `proc`, a sequence of list positions, and divides each node of it.  Round A: every node with more than one key,
//     front to back.  Round B: the nodes of E (the children with more than one key the last round created, in creation order) sorted
//     ascending by (key count, UL.x, position in E) and walked from the back, until the list holds N nodes;
//   * the new list is the non-empty children in reverse creation order followed by the nodes that were not divided in their old order;
//   * a node's keys are a run [begin, begin + count) of a permutation of the input indices; a division partitions the run stably into
//     its four quadrants, so key order inside a node is always input order.
//
// Loop bounds.  Round r divides only nodes created in round r - 1 (the roots in round 1), so every node a round divides has depth
// r - 1, and a box of depth d is at most ceil(side / 2^d) wide and high.  With side <= kOctMaxSide = 2^15 a box of depth 15 is at most
// one pixel wide and high; dividing such a box compares every key with the same mx = UR.x and my = BL.y that its children will compare
// with again, so round 16 can still separate keys that lie outside their box from those inside, and from round 17 on no division
// puts the keys of a node into more than one child: the list stops growing and the `size == prevSize` rule ends the walk.  No list
// needs more than 17 rounds; kOctMaxRounds = 20 is the counted bound, and a list that reaches it is reported, not continued.  The
// list never holds more than max(N + 3, 4 * nIni) nodes: a round A is only entered with size + 3 |E| <= N (or from the roots), and a
// round B stops at the first division that reaches N, which adds at most 3.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OSH_OCT_HD __host__ __device__ inline
#else
#define OSH_OCT_HD inline
#endif

namespace osh {

constexpr int kOctMaxSide = 32768;        // OSH_FAST_MAX_SIDE: W and H
constexpr int kOctMaxFeatures = 2048;     // OSH_OCTREE_MAX_FEATURES: N of a list
constexpr int kOctMaxKeys = 1 << 16;      // OSH_OCTREE_MAX_CANDIDATES: an input index fits 16 bits
constexpr int kOctMaxRoots = 64;          // OSH_OCTREE_MAX_ROOTS: nIni, an area 64 times as wide as high.  The first round leaves up to 4 nIni
                                          // nodes whatever N is, and the kernel places the roots with nIni passes over the keys
constexpr int kOctMaxNodes = 2304;        // >= max(kOctMaxFeatures + 3, 4 * kOctMaxRoots), a multiple of 256
constexpr int kOctMaxRounds = 20;         // see above
static_assert(kOctMaxNodes >= kOctMaxFeatures + 3 && kOctMaxNodes >= 4 * kOctMaxRoots, "the list fits");

struct OctBox { int ulx, urx, uly, bry; };   // columns [UL.x, UR.x), rows [UL.y, BL.y)

// nIni = round((float)W / (float)H), halves away from zero; 0 (W < H / 2, where the reference divides by zero) is taken as 1
OSH_OCT_HD int oct_n_ini(int W, int H) {
  const int r = (int)roundf((float)W / (float)H);
  return r == 0 ? 1 : r;
}
OSH_OCT_HD float oct_hx(int W, int n_ini) { return (float)W / (float)n_ini; }
OSH_OCT_HD OctBox oct_root(float hx, int i, int H) { return {(int)(hx * (float)i), (int)(hx * (float)(i + 1)), 0, H}; }
// the root of a key: (int)(x / hX); an index equal to nIni (the reference indexes past its vector) is taken as nIni - 1
OSH_OCT_HD int oct_root_of(float x, float hx, int n_ini) {
  const int r = (int)(x / hx);
  return r >= n_ini ? n_ini - 1 : r;
}

OSH_OCT_HD int oct_half(int d) { return (int)ceilf((float)d / 2.f); }
OSH_OCT_HD void oct_mid(const OctBox& b, int& mx, int& my) { mx = b.ulx + oct_half(b.urx - b.ulx); my = b.uly + oct_half(b.bry - b.uly); }
// 0: n1 left-top, 1: n2 right-top, 2: n3 left-bottom, 3: n4 right-bottom.  Nothing else is tested: a key outside its box is legal.
OSH_OCT_HD int oct_quadrant(float x, float y, int mx, int my) { return (x < (float)mx ? 0 : 1) + (y < (float)my ? 0 : 2); }
OSH_OCT_HD OctBox oct_child(const OctBox& b, int mx, int my, int q) {
  return {(q & 1) ? mx : b.ulx, (q & 1) ? b.urx : mx, (q & 2) ? my : b.uly, (q & 2) ? b.bry : my};
}

// Round B sorts E ascending by this key: unique, so any sort gives the stable order of (count, UL.x)
OSH_OCT_HD uint64_t oct_sort_key(int count, int ulx, int pos_in_e) { return ((uint64_t)(uint32_t)count << 32) | ((uint64_t)(uint32_t)ulx << 16) | (uint32_t)pos_in_e; }
// Round B walks the sorted E from the back and breaks as soon as the list holds N nodes: its t-th node (t = 0 first) is divided
// when the list, after the t divisions before it with `created_before` non-empty children, is still shorter than N
OSH_OCT_HD bool oct_b_walks(int size, int created_before, int t, int N) { return size + created_before - t < N; }

// The winner of a node is the maximum of this key over its keys: the largest response, and among equal responses the smallest
// input index (-0 counts as +0, as in a float comparison; the response is finite)
OSH_OCT_HD uint64_t oct_winner_key(float response, uint32_t index) {
  const float r = response + 0.f;
  uint32_t u;
  memcpy(&u, &r, 4);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint32_t)~index;
}
OSH_OCT_HD uint32_t oct_winner_index(uint64_t key) { return ~(uint32_t)key; }

// ---- host only

enum { kOctOk = 0, kOctInvalid = -1, kOctUnsupported = -3, kOctRoundBound = -2 };   // OSH_OK, OSH_ERR_INVALID, OSH_ERR_UNSUPPORTED, OSH_ERR_DEVICE

// What osh_orb_octree_distribute refuses of one list, in its order; *why names the reason
inline int oct_validate_list(int n, const float* xy, const float* response, int W, int H, int N, const char** why) {
  if (n < 0) { *why = "negative candidate count"; return kOctInvalid; }
  if (n && (!xy || !response)) { *why = "NULL candidate array with a non-zero count"; return kOctInvalid; }
  if (W <= 0 || H <= 0 || W > kOctMaxSide || H > kOctMaxSide) { *why = "width or height outside [1, OSH_FAST_MAX_SIDE]"; return kOctInvalid; }
  if (N > kOctMaxFeatures) { *why = "more than OSH_OCTREE_MAX_FEATURES features"; return kOctUnsupported; }
  if (n > kOctMaxKeys) { *why = "more than OSH_OCTREE_MAX_CANDIDATES candidates"; return kOctUnsupported; }
  if (oct_n_ini(W, H) > kOctMaxRoots) { *why = "more than OSH_OCTREE_MAX_ROOTS roots"; return kOctUnsupported; }
  for (int k = 0; k < n; ++k) {
    const float x = xy[2 * k], y = xy[2 * k + 1];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(response[k])) { *why = "a candidate is not finite"; return kOctInvalid; }
    if (!(x >= 0.f) || !(x < (float)W) || !(y >= 0.f)) { *why = "a candidate has x outside [0, width) or a negative y"; return kOctInvalid; }
  }
  return kOctOk;
}

struct OctNodeHost { OctBox box; int begin, count; };   // keys: perm[begin, begin + count)

// One list on one thread: the kept input indices in result order.  No limit on n, N or nIni; the inputs must pass the finite and
// range checks of oct_validate_list.  kOctRoundBound if the round bound is reached (it cannot be, see above).
inline int octree_distribute_host(int n, const float* xy, const float* response, int W, int H, int N, std::vector<int>& kept) {
  kept.clear();
  const int n_ini = oct_n_ini(W, H);
  const float hx = oct_hx(W, n_ini);
  std::vector<int> perm(n), tmp(n), root_of(n), root_begin((size_t)n_ini + 1, 0);
  for (int k = 0; k < n; ++k) { root_of[k] = oct_root_of(xy[2 * k], hx, n_ini); ++root_begin[root_of[k] + 1]; }
  for (int i = 0; i < n_ini; ++i) root_begin[i + 1] += root_begin[i];
  {
    std::vector<int> at(root_begin.begin(), root_begin.end() - 1);
    for (int k = 0; k < n; ++k) perm[at[root_of[k]]++] = k;
  }
  std::vector<OctNodeHost> list, created, next;   // front to back
  for (int i = 0; i < n_ini; ++i)
    if (root_begin[i + 1] > root_begin[i]) list.push_back({oct_root(hx, i, H), root_begin[i], root_begin[i + 1] - root_begin[i]});
  std::vector<int> E, proc, e_created;            // E: positions in `list`, in creation order
  std::vector<char> gone;
  bool mode_b = false, finished = false;
  for (int round = 0; round < kOctMaxRounds && !finished; ++round) {
    const int S = (int)list.size();
    proc.clear();
    if (!mode_b) {
      for (int p = 0; p < S; ++p) if (list[p].count > 1) proc.push_back(p);
    } else {
      std::vector<int> order(E.size());
      std::iota(order.begin(), order.end(), 0);
      std::sort(order.begin(), order.end(), [&](int a, int b) {
        return oct_sort_key(list[E[a]].count, list[E[a]].box.ulx, a) < oct_sort_key(list[E[b]].count, list[E[b]].box.ulx, b);
      });
      for (size_t j = order.size(); j-- > 0;) proc.push_back(E[order[j]]);
    }
    created.clear(); e_created.clear();
    gone.assign(S, 0);
    for (int t = 0; t < (int)proc.size(); ++t) {
      if (mode_b && !oct_b_walks(S, (int)created.size(), t, N)) break;
      const OctNodeHost nd = list[proc[t]];
      int mx, my;
      oct_mid(nd.box, mx, my);
      int c[4] = {0, 0, 0, 0}, at[4];
      for (int k = nd.begin; k < nd.begin + nd.count; ++k) ++c[oct_quadrant(xy[2 * perm[k]], xy[2 * perm[k] + 1], mx, my)];
      at[0] = nd.begin; at[1] = at[0] + c[0]; at[2] = at[1] + c[1]; at[3] = at[2] + c[2];
      for (int q = 0; q < 4; ++q) {
        if (!c[q]) continue;
        if (c[q] > 1) e_created.push_back((int)created.size());
        created.push_back({oct_child(nd.box, mx, my, q), at[q], c[q]});
      }
      for (int k = nd.begin; k < nd.begin + nd.count; ++k) tmp[at[oct_quadrant(xy[2 * perm[k]], xy[2 * perm[k] + 1], mx, my)]++] = perm[k];
      std::copy(tmp.begin() + nd.begin, tmp.begin() + nd.begin + nd.count, perm.begin() + nd.begin);
      gone[proc[t]] = 1;
    }
    const int C = (int)created.size();
    next.clear();
    for (int r = C; r-- > 0;) next.push_back(created[r]);
    for (int p = 0; p < S; ++p) if (!gone[p]) next.push_back(list[p]);
    list.swap(next);
    E.clear();
    for (int idx : e_created) E.push_back(C - 1 - idx);
    const int size = (int)list.size();
    if (size >= N || size == S) finished = true;
    else if (!mode_b && size + 3 * (int)E.size() > N) mode_b = true;
  }
  if (!finished) return kOctRoundBound;
  kept.reserve(list.size());
  for (const OctNodeHost& nd : list) {
    uint64_t best = 0;
    for (int k = nd.begin; k < nd.begin + nd.count; ++k) best = std::max(best, oct_winner_key(response[perm[k]], (uint32_t)perm[k]));
    kept.push_back((int)oct_winner_index(best));
  }
  return kOctOk;
}

}  // namespace osh
