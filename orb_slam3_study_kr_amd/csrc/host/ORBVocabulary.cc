// ORBVocabulary.cc -- ORB_SLAM3::ORBVocabulary (include/ORBVocabulary.h): the text loader of
// Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1337-1424, transform (:1127-1194) as a pack and a write-back around
// osh_orb_bow_transform (csrc/bow_device.hip), and L1Scoring::score (ScoringObject.cpp:23-68) on the host.  It replaces
// Thirdparty/DBoW2's transform for Frame::ComputeBoW and KeyFrame::ComputeBoW, whose reference bodies call it unchanged.
// There is no CPU fallback.
//
// Intended deviations from the reference:
//   * the loader skips empty lines: the reference's `while(!f.eof())` turns the trailing newline of the file into one more child of
//     the root with an unset descriptor;
//   * a feature whose leaf lies above depth L - levelsup is filed under the leaf itself: the reference leaves nid uninitialised.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include "ORBVocabulary.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // csrc/host/ORBmatcher.cc
int HostMatcherDevice();

ORBVocabulary::~ORBVocabulary() { ReleaseDevice(); }

void ORBVocabulary::ReleaseDevice() {
  std::lock_guard<std::mutex> lock(mMutexDevice);
  for (auto& dv : mDeviceVocab) osh_bow_vocab_destroy(dv.second);
  mDeviceVocab.clear();
}

osh_bow_tree ORBVocabulary::Tree() const {
  osh_bow_tree t;
  t.k = mK; t.L = mL; t.weighting = mWeighting; t.scoring = mScoring;
  t.n = (int32_t)mParent.size();
  t.parent = mParent.data(); t.is_leaf = mIsLeaf.data(); t.desc = mDesc.data(); t.weight = mWeight.data();
  return t;
}

bool ORBVocabulary::loadFromTextFile(const std::string& filename) {
  ReleaseDevice();
  mK = mL = mScoring = mWeighting = 0;
  mParent.clear(); mIsLeaf.clear(); mDesc.clear(); mWeight.clear(); mWordNode.clear();
  std::ifstream f(filename.c_str());
  std::string line;
  if (!f.is_open() || !std::getline(f, line)) return false;
  int k = -1, L = -1, n1 = -1, n2 = -1;
  if (std::sscanf(line.c_str(), "%d %d %d %d", &k, &L, &n1, &n2) != 4 || k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) {   // :1359
    std::fprintf(stderr, "Vocabulary loading failure: This is not a correct text file!\n");
    return false;
  }
  std::vector<int32_t> parent, word_node;
  std::vector<uint8_t> is_leaf, desc;
  std::vector<double> weight;
  while (std::getline(f, line)) {
    const char* p = line.c_str();
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    char* end = nullptr;
    long field[34];
    bool ok = true;
    for (int i = 0; i < 34 && ok; ++i) { field[i] = std::strtol(p, &end, 10); ok = end != p; p = end; }
    const double w = ok ? std::strtod(p, &end) : 0.0;
    if (!ok || end == p) {
      std::fprintf(stderr, "Vocabulary loading failure: node line %zu is malformed\n", parent.size() + 2);
      return false;
    }
    parent.push_back((int32_t)field[0]);
    is_leaf.push_back(field[1] > 0 ? 1 : 0);
    for (int i = 0; i < 32; ++i) desc.push_back((uint8_t)field[2 + i]);
    weight.push_back(w);
    if (field[1] > 0) word_node.push_back((int32_t)parent.size());   // words in file order (:1408-1415)
  }
  mK = k; mL = L; mScoring = n1; mWeighting = n2;
  mParent.swap(parent); mIsLeaf.swap(is_leaf); mDesc.swap(desc); mWeight.swap(weight); mWordNode.swap(word_node);
  const osh_bow_tree t = Tree();
  if (osh_bow_tree_check(&t) != OSH_OK) {
    std::fprintf(stderr, "Vocabulary loading failure: %s\n", osh_last_error());
    mParent.clear(); mIsLeaf.clear(); mDesc.clear(); mWeight.clear(); mWordNode.clear();
    return false;
  }
  return true;
}

DBoW2::NodeId ORBVocabulary::getParentNode(DBoW2::WordId wid, int levelsup) const {
  int ret = mWordNode[wid];
  while (levelsup > 0 && ret != 0) { --levelsup; ret = mParent[ret - 1]; }
  return (DBoW2::NodeId)ret;
}

double ORBVocabulary::score(const DBoW2::BowVector& v1, const DBoW2::BowVector& v2) const {
#pragma clang fp contract(off)
  auto it1 = v1.begin(), it2 = v2.begin();
  double score = 0;
  while (it1 != v1.end() && it2 != v2.end()) {
    const double vi = it1->second, wi = it2->second;
    if (it1->first == it2->first) {
      score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
      ++it1; ++it2;
    } else if (it1->first < it2->first) {
      it1 = v1.lower_bound(it2->first);
    } else {
      it2 = v2.lower_bound(it1->first);
    }
  }
  return -score / 2.0;
}

void ORBVocabulary::transform(const std::vector<cv::Mat>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const {
  std::vector<uint8_t> desc(features.size() * 32);
  for (size_t i = 0; i < features.size(); ++i) std::memcpy(&desc[32 * i], features[i].ptr<uint8_t>(0), 32);
  transform(desc.data(), (int)features.size(), v, fv, levelsup);
}

void ORBVocabulary::transform(const cv::Mat& descriptors, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const {
  const int n = descriptors.rows;
  if (n > 0 && descriptors.step == 32) { transform(descriptors.ptr<uint8_t>(0), n, v, fv, levelsup); return; }
  std::vector<uint8_t> desc((size_t)n * 32);
  for (int i = 0; i < n; ++i) std::memcpy(&desc[32 * (size_t)i], descriptors.ptr<uint8_t>(i), 32);
  transform(desc.data(), n, v, fv, levelsup);
}

void ORBVocabulary::transform(const uint8_t* desc, int n, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const {
  v.clear();
  fv.clear();
  if (empty() || n <= 0) return;   // :1134
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) {
    std::fprintf(stderr, "ORBVocabulary::transform: %s\n", osh_last_error());
    return;
  }
  const int device = HostMatcherDevice();
  osh_bow_vocab* vocab = nullptr;
  {
    std::lock_guard<std::mutex> lock(mMutexDevice);
    auto it = mDeviceVocab.find(device);
    if (it == mDeviceVocab.end()) {
      const osh_bow_tree t = Tree();
      if (osh_bow_vocab_create(device, &t, &vocab) != OSH_OK) {
        std::fprintf(stderr, "ORBVocabulary::transform: %s\n", osh_last_error());
        return;
      }
      mDeviceVocab[device] = vocab;
    } else {
      vocab = it->second;
    }
  }
  int32_t n_words = 0, n_nodes = 0;
  std::vector<int32_t> word_id(n), node_id(n), node_start((size_t)n + 1), node_feat(n);
  std::vector<double> word_value(n);
  const osh_bow_frame frame{n, desc};
  const osh_bow_result res{&n_words, word_id.data(), word_value.data(), &n_nodes, node_id.data(), node_start.data(), node_feat.data(),
                           nullptr, nullptr, nullptr};
  if (osh_orb_bow_transform(ctx, vocab, levelsup, 1, &frame, &res) != OSH_OK) {
    std::fprintf(stderr, "ORBVocabulary::transform: %s\n", osh_last_error());
    return;
  }
  for (int a = 0; a < n_words; ++a) v.insert(v.end(), DBoW2::BowVector::value_type((unsigned)word_id[a], word_value[a]));
  for (int a = 0; a < n_nodes; ++a)
    fv.insert(fv.end(), DBoW2::FeatureVector::value_type((unsigned)node_id[a], std::vector<unsigned int>(node_feat.begin() + node_start[a],
                                                                                                         node_feat.begin() + node_start[a + 1])));
}

}  // namespace ORB_SLAM3
