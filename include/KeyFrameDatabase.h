/* KeyFrameDatabase.h -- ORB_SLAM3::KeyFrameDatabase (reference include/KeyFrameDatabase.h:47-99) with the inverted file on the
 * device: csrc/host/KeyFrameDatabase.cc around osh_bow_db and osh_orb_bow_db_query (csrc/bowdb_device.hip).  add, erase, clear and
 * clearMap keep one device row per keyframe; DetectNBestCandidates (LoopClosing) and DetectRelocalizationCandidates (Tracking)
 * are the reference's bodies statement by statement, with the walk over the inverted lists and the L1 scores replaced by one
 * device query.  Candidates, their order and all six marker fields of every keyframe equal the reference's.
 *
 * Not provided: DetectLoopCandidates, DetectCandidates and DetectBestCandidates (no caller in the reference), PreSave, PostLoad
 * and serialize (Atlas save / load).
 *
 * One object serves Tracking, LoopClosing and LocalMapping (KeyFrame::SetBadFlag) at once under its mutex; the device database is
 * made on the first add or query, on the device of the matcher contexts, and each query runs on the calling thread's matcher
 * context. */
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>
#include "Frame.h"
#include "KeyFrame.h"
#include "Map.h"
#include "ORBVocabulary.h"
#include "orbslam3_hip.h"

namespace ORB_SLAM3 {
class KeyFrameDatabase {
 public:
  KeyFrameDatabase() {}
  // a vocabulary whose scoring is not L1_NORM is refused with a message on stderr: the database then stays empty and finds nothing
  KeyFrameDatabase(const ORBVocabulary& voc);
  ~KeyFrameDatabase();
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  // A keyframe with an empty mBowVec adds no row (in the reference it enters no list).  Intended deviation: a keyframe that is
  // already present is refused with a message on stderr; the reference would enter it twice and double its counts.
  void add(KeyFrame* pKF);
  void erase(KeyFrame* pKF);
  void clear();
  void clearMap(Map* pMap);

  // src/KeyFrameDatabase.cc:604-730.  Intended deviation: a bad keyframe in the sorted list is skipped (:712 of the reference
  // never advances and loops forever).  On a device error: osh_last_error() on stderr, no candidate and no marker touched.
  void DetectNBestCandidates(KeyFrame* pKF, std::vector<KeyFrame*>& vpLoopCand, std::vector<KeyFrame*>& vpMergeCand, int nNumCandidates);
  // src/KeyFrameDatabase.cc:733-845
  std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F, Map* pMap);

  void SetORBVocabulary(ORBVocabulary* pORBVoc);   // :847-852; the database is empty afterwards

 protected:
  struct Listed { KeyFrame* pKF; int words; bool scored; double score; };
  bool Usable(const char* who);
  // The device query for `bow` with the keyframes of `excluded` left out: the rows that share a word, in the order in which the
  // reference's walk first meets them.  false on a device error
  bool Query(const DBoW2::BowVector& bow, const std::vector<uint64_t>& excluded, std::vector<Listed>& rows);

  const ORBVocabulary* mpVoc = nullptr;
  bool mbRefused = false;
  std::mutex mMutex;
  osh_bow_db* mpDb = nullptr;
  std::map<uint64_t, KeyFrame*> mKeyFrames;   // by handle: add order
  std::map<KeyFrame*, uint64_t> mHandles;
};
}  // namespace ORB_SLAM3
#endif
