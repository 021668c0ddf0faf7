/* ORBVocabulary.h -- ORB_SLAM3::ORBVocabulary (reference include/ORBVocabulary.h: a typedef of
 * DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) as a class whose transform runs on the device (csrc/host/ORBVocabulary.cc
 * around osh_orb_bow_transform, csrc/bow_device.hip).  It carries the members ORB-SLAM3 calls: the text loader, the two-vector
 * transform, the L1 score and the bookkeeping getters.  Training (create), the binary and YAML loaders and the other scores are
 * not here.
 *
 * One object serves Tracking, LocalMapping and LoopClosing at once: it is immutable after loadFromTextFile, its device copy is made
 * on the first transform of a device (under a mutex) and shared from then on, and each transform runs on the calling thread's
 * matcher context. */
#ifndef ORBVOCABULARY_H
#define ORBVOCABULARY_H
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "orbslam3_compat.h"
#include "orbslam3_hip.h"

#ifdef ORBSLAM3_HIP_USE_REAL_HEADERS
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"       /* the tree's own map types and enums, as its ORBVocabulary.h includes them */
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
#else
namespace DBoW2 {
typedef unsigned int WordId;
typedef unsigned int NodeId;
typedef double WordValue;
enum WeightingType { TF_IDF, TF, IDF, BINARY };                                         /* BowVector.h:39-45 */
enum ScoringType { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };      /* BowVector.h:48-56 */
}  // namespace DBoW2
#endif

namespace ORB_SLAM3 {
class ORBVocabulary {
 public:
  ORBVocabulary() {}
  ~ORBVocabulary();
  ORBVocabulary(const ORBVocabulary&) = delete;
  ORBVocabulary& operator=(const ORBVocabulary&) = delete;

  // TemplatedVocabulary.h:1337-1424: first line `k L scoring weighting`, then one line `parent leaf d0 .. d31 weight` per node.
  // Empty lines are skipped (the reference turns a trailing newline into one more child of the root).  false, with a message on
  // stderr, for a file that does not open, a first line outside the loader's limits, a malformed node line or a tree
  // osh_bow_tree_check refuses; the vocabulary is then empty.
  bool loadFromTextFile(const std::string& filename);
  // :1127-1194 on the device.  On a device error: osh_last_error() on stderr and both vectors empty.
  void transform(const std::vector<cv::Mat>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const;
  // the same for the N x 32 descriptor matrix of a frame (what Converter::toDescriptorVector splits into rows)
  void transform(const cv::Mat& descriptors, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const;
  // L1Scoring::score (ScoringObject.cpp:23-68) on the host, in its merge order
  double score(const DBoW2::BowVector& a, const DBoW2::BowVector& b) const;

  bool empty() const { return mWordNode.empty(); }
  unsigned int size() const { return (unsigned int)mWordNode.size(); }
  int getBranchingFactor() const { return mK; }
  int getDepthLevels() const { return mL; }
  DBoW2::WeightingType getWeightingType() const { return (DBoW2::WeightingType)mWeighting; }
  DBoW2::ScoringType getScoringType() const { return (DBoW2::ScoringType)mScoring; }
  DBoW2::NodeId getParentNode(DBoW2::WordId wid, int levelsup) const;   // :1263-1274

  // the loaded tree in the C-ABI's form (nodes 1..n in file order); the pointers live as long as the object is not reloaded
  osh_bow_tree Tree() const;

 private:
  void transform(const uint8_t* desc, int n, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const;
  void ReleaseDevice();
  int mK = 0, mL = 0, mScoring = 0, mWeighting = 0;
  std::vector<int32_t> mParent;
  std::vector<uint8_t> mIsLeaf, mDesc;
  std::vector<double> mWeight;
  std::vector<int32_t> mWordNode;                     // node id of each word
  mutable std::mutex mMutexDevice;
  mutable std::map<int, osh_bow_vocab*> mDeviceVocab;  // by device
};
}  // namespace ORB_SLAM3
#endif
