// bow.cc -- the osh_host_bow_* wrappers of include/orbslam3_hip_host.h: a plain single-thread C++ restatement of
// TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259) with std::map vectors like the reference's
// (the CPU baseline of profiles/bow_timing.py), an ORBVocabulary loaded from a text file behind a handle, Frame::ComputeBoW /
// KeyFrame::ComputeBoW on stand-ins built from flat arrays, and ORBVocabulary::score.  The stand-in bodies of the two ComputeBoW
// live here as well: an integrator keeps the reference's, which call ORBVocabulary::transform unchanged.  Test library only.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <thread>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "Map.h"
#include "ORBVocabulary.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

namespace ORB_SLAM3 {

// src/Frame.cc:737-744
void Frame::ComputeBoW() {
  if (mBowVec.empty()) mpORBvocabulary->transform(mDescriptors, mBowVec, mFeatVec, 4);
}

// src/KeyFrame.cc:92-102
void KeyFrame::ComputeBoW() {
  if (mBowVec.empty() || mFeatVec.empty()) mpORBvocabulary->transform(mDescriptors, mBowVec, mFeatVec, 4);
}

}  // namespace ORB_SLAM3

using namespace ORB_SLAM3;

namespace {

inline int hamming256(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int k = 0; k < 4; ++k) {
    uint64_t x, y;
    std::memcpy(&x, a + 8 * k, 8); std::memcpy(&y, b + 8 * k, 8);
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}

// the two maps as the arrays of an osh_bow_result
void flatten(const DBoW2::BowVector& v, const DBoW2::FeatureVector& fv, const osh_bow_result* out) {
  int a = 0;
  for (const auto& e : v) {
    if (out->word_id) out->word_id[a] = (int32_t)e.first;
    if (out->word_value) out->word_value[a] = e.second;
    ++a;
  }
  if (out->n_words) *out->n_words = a;
  int b = 0, t = 0;
  for (const auto& e : fv) {
    if (out->node_id) out->node_id[b] = (int32_t)e.first;
    if (out->node_start) out->node_start[b] = t;
    for (unsigned int i : e.second) { if (out->node_feat) out->node_feat[t] = (int32_t)i; ++t; }
    ++b;
  }
  if (out->node_start) out->node_start[b] = t;
  if (out->n_nodes) *out->n_nodes = b;
}

struct Node {
  std::vector<int> children;
  double weight = 0;
  int word_id = -1;
};

}  // namespace

struct osh_host_bow_vocab { ORBVocabulary voc; };

extern "C" int osh_host_bow_restatement(const osh_bow_tree* t, int32_t levelsup, int32_t n, const uint8_t* desc, const osh_bow_result* out, double* ms) {
#pragma clang fp contract(off)
  if (!out || n < 0 || (n && !desc) || osh_bow_tree_check(t) != OSH_OK) return -1;
  if (t->scoring == OSH_BOW_L2_NORM) return -2;
  std::vector<Node> nodes((size_t)t->n + 1);   // the loader, :1376-1420
  int n_words = 0;
  for (int i = 0; i < t->n; ++i) {
    const int nid = i + 1;
    nodes[t->parent[i]].children.push_back(nid);
    nodes[nid].weight = t->weight[i];
    if (t->is_leaf[i] > 0) nodes[nid].word_id = n_words++;
  }
  const auto t0 = std::chrono::steady_clock::now();
  DBoW2::BowVector v;
  DBoW2::FeatureVector fv;
  const bool sums = t->weighting == OSH_BOW_TF || t->weighting == OSH_BOW_TF_IDF;
  const bool must = t->scoring != OSH_BOW_DOT_PRODUCT;
  const int nid_level = t->L - levelsup;
  for (int i = 0; i < n; ++i) {
    const uint8_t* feature = desc + 32 * (size_t)i;
    int nid = 0, final_id = 0, current_level = 0, best_d = 0;
    bool nid_set = nid_level <= 0;   // :1227
    do {
      ++current_level;
      const std::vector<int>& ch = nodes[final_id].children;
      final_id = ch[0];
      best_d = hamming256(feature, t->desc + 32 * (size_t)(final_id - 1));
      for (size_t c = 1; c < ch.size(); ++c) {
        const int d = hamming256(feature, t->desc + 32 * (size_t)(ch[c] - 1));
        if (d < best_d) { best_d = d; final_id = ch[c]; }
      }
      if (current_level == nid_level) { nid = final_id; nid_set = true; }
    } while (!nodes[final_id].children.empty());
    if (!nid_set) nid = final_id;    // the intended deviation: a leaf above the level records itself
    const int id = nodes[final_id].word_id;
    const double w = nodes[final_id].weight;
    if (out->feat_word) out->feat_word[i] = id;
    if (out->feat_node) out->feat_node[i] = nid;
    if (out->feat_dist) out->feat_dist[i] = best_d;
    if (w > 0) {
      auto vit = v.lower_bound((unsigned)id);
      if (vit != v.end() && vit->first == (unsigned)id) { if (sums) vit->second += w; }
      else v.insert(vit, DBoW2::BowVector::value_type((unsigned)id, w));
      fv[(unsigned)nid].push_back((unsigned)i);
    }
  }
  if (sums && !v.empty() && !must) {
    const double nd = (double)v.size();
    for (auto& e : v) e.second /= nd;
  }
  if (must) {
    double norm = 0.0;
    for (const auto& e : v) norm += std::fabs(e.second);
    if (norm > 0.0) for (auto& e : v) e.second /= norm;
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  flatten(v, fv, out);
  return 0;
}

extern "C" osh_host_bow_vocab* osh_host_bow_vocab_load(const char* path) {
  if (!path) return nullptr;
  osh_host_bow_vocab* h = new osh_host_bow_vocab();
  if (!h->voc.loadFromTextFile(path)) { delete h; return nullptr; }
  return h;
}

extern "C" void osh_host_bow_vocab_free(osh_host_bow_vocab* h) { delete h; }

extern "C" int osh_host_bow_vocab_tree(const osh_host_bow_vocab* h, int32_t info[7], int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight,
                                       int32_t levelsup, int32_t* word_parent) {
  if (!h || !info) return -1;
  const ORBVocabulary& V = h->voc;
  const osh_bow_tree t = V.Tree();
  info[0] = V.getBranchingFactor(); info[1] = V.getDepthLevels(); info[2] = (int32_t)V.getWeightingType(); info[3] = (int32_t)V.getScoringType();
  info[4] = t.n; info[5] = (int32_t)V.size(); info[6] = V.empty() ? 1 : 0;
  if (parent) std::memcpy(parent, t.parent, sizeof(int32_t) * (size_t)t.n);
  if (is_leaf) std::memcpy(is_leaf, t.is_leaf, (size_t)t.n);
  if (desc) std::memcpy(desc, t.desc, (size_t)t.n * 32);
  if (weight) std::memcpy(weight, t.weight, sizeof(double) * (size_t)t.n);
  if (word_parent) for (unsigned w = 0; w < V.size(); ++w) word_parent[w] = (int32_t)V.getParentNode(w, levelsup);
  return 0;
}

extern "C" int osh_host_bow_compute(osh_host_bow_vocab* h, int32_t keyframe, int32_t n, const uint8_t* desc, const uint8_t* second_desc,
                                    int32_t n_threads, const osh_bow_result* out) {
  if (!h || n < 0 || (n && !desc) || n_threads < 1 || !out) return -1;
  auto matrix = [n](const uint8_t* d) {
    cv::Mat m(n, 32);
    if (n) std::memcpy(m.ptr<uint8_t>(0), d, (size_t)n * 32);
    return m;
  };
  auto run = [&](DBoW2::BowVector& v, DBoW2::FeatureVector& fv) {
    Map map;
    Frame F;
    KeyFrame K(0, &map);
    if (keyframe) { K.mDescriptors = matrix(desc); K.mpORBvocabulary = &h->voc; K.ComputeBoW(); }
    else { F.mDescriptors = matrix(desc); F.mpORBvocabulary = &h->voc; F.ComputeBoW(); }
    if (second_desc) {   // the guard: other descriptors, the vectors stay
      if (keyframe) { K.mDescriptors = matrix(second_desc); K.ComputeBoW(); }
      else { F.mDescriptors = matrix(second_desc); F.ComputeBoW(); }
    }
    v = keyframe ? K.mBowVec : F.mBowVec;
    fv = keyframe ? K.mFeatVec : F.mFeatVec;
  };
  std::vector<DBoW2::BowVector> v(n_threads);
  std::vector<DBoW2::FeatureVector> fv(n_threads);
  if (n_threads == 1) {
    run(v[0], fv[0]);
  } else {           // every thread on its own matcher context, all on the one vocabulary
    std::vector<std::thread> pool;
    for (int k = 0; k < n_threads; ++k) pool.emplace_back([&, k] { run(v[k], fv[k]); });
    for (auto& th : pool) th.join();
    for (int k = 1; k < n_threads; ++k) if (v[k] != v[0] || fv[k] != fv[0]) return -3;
  }
  flatten(v[0], fv[0], out);
  return 0;
}

extern "C" double osh_host_bow_score(int32_t n1, const int32_t* id1, const double* value1, int32_t n2, const int32_t* id2, const double* value2) {
  DBoW2::BowVector a, b;
  for (int i = 0; i < n1; ++i) a[(unsigned)id1[i]] = value1[i];
  for (int i = 0; i < n2; ++i) b[(unsigned)id2[i]] = value2[i];
  return ORBVocabulary().score(a, b);
}
