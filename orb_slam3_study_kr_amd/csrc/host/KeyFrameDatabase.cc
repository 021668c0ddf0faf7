// KeyFrameDatabase.cc -- ORB_SLAM3::KeyFrameDatabase (include/KeyFrameDatabase.h): src/KeyFrameDatabase.cc:32-98 and 604-845 with the
// inverted file kept on the device (osh_bow_db, csrc/bowdb_device.hip).  The two Detect bodies are the reference's, statement by
// statement; only the walk over the inverted lists and the calls of mpVoc->score are replaced by one osh_orb_bow_db_query.
// There is no CPU fallback.
//
// Why the result order is the reference's: every inverted list holds its keyframes in add order, and the walk takes the query's
// words ascending.  So the walk first meets a keyframe at the smallest word they share, and two keyframes that share the same
// smallest word are met in add order.  The device returns that word per row and handles ascend in add order: sorting the rows by
// (first word, handle) gives lKFsSharingWords.  The keyframes the reference keeps out of that list (the connected ones, and those
// whose marker already equals the query id) are excluded from the maximum and the scores on the device and get the reference's
// marker updates from their counts here.
//
// Intended deviations from the reference:
//   * add of a keyframe that is already present is refused with a message (the reference would double its counts; no caller does it);
//   * `if(pKFi->isBad()) continue;` at :712 never advances and loops forever: here a bad keyframe is skipped and the walk goes on.
#include <algorithm>
#include <cstdio>
#include <list>
#include <set>
#include "KeyFrameDatabase.h"

namespace ORB_SLAM3 {

osh_orb_ctx* HostMatcherContext();   // csrc/host/ORBmatcher.cc
int HostMatcherDevice();

namespace {

void flatten(const DBoW2::BowVector& v, std::vector<int32_t>& id, std::vector<double>& value) {
  id.clear(); value.clear();
  for (const auto& e : v) { id.push_back((int32_t)e.first); value.push_back(e.second); }
}

bool compFirst(const std::pair<float, KeyFrame*>& a, const std::pair<float, KeyFrame*>& b) { return a.first > b.first; }   // :598-601

}  // namespace

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc) {
  if (voc.getScoringType() != DBoW2::L1_NORM) {
    std::fprintf(stderr, "KeyFrameDatabase: the vocabulary's scoring type %d is not L1_NORM; the database stays empty\n", (int)voc.getScoringType());
    mbRefused = true;
  }
}

KeyFrameDatabase::~KeyFrameDatabase() {
  if (mpDb) osh_bow_db_destroy(mpDb);
}

// mMutex held.  The device database, made on first use
bool KeyFrameDatabase::Usable(const char* who) {
  if (mbRefused || !mpVoc) return false;
  if (mpDb) return true;
  if (osh_bow_db_create(HostMatcherDevice(), (int64_t)mpVoc->size(), &mpDb) != OSH_OK) {
    std::fprintf(stderr, "KeyFrameDatabase::%s: %s\n", who, osh_last_error());
    mpDb = nullptr;
    return false;
  }
  return true;
}

void KeyFrameDatabase::add(KeyFrame* pKF) {
  std::unique_lock<std::mutex> lock(mMutex);
  if (pKF->mBowVec.empty()) return;
  if (mHandles.count(pKF)) {
    std::fprintf(stderr, "KeyFrameDatabase::add: keyframe %lu is already in the database; not added again\n", pKF->mnId);
    return;
  }
  if (!Usable("add")) return;
  std::vector<int32_t> id;
  std::vector<double> value;
  flatten(pKF->mBowVec, id, value);
  uint64_t handle = 0;
  if (osh_bow_db_add(mpDb, (int32_t)id.size(), id.data(), value.data(), &handle) != OSH_OK) {
    std::fprintf(stderr, "KeyFrameDatabase::add: %s\n", osh_last_error());
    return;
  }
  mKeyFrames[handle] = pKF;
  mHandles[pKF] = handle;
}

void KeyFrameDatabase::erase(KeyFrame* pKF) {
  std::unique_lock<std::mutex> lock(mMutex);
  const auto it = mHandles.find(pKF);
  if (it == mHandles.end()) return;
  if (osh_bow_db_erase(mpDb, it->second) != OSH_OK) std::fprintf(stderr, "KeyFrameDatabase::erase: %s\n", osh_last_error());
  mKeyFrames.erase(it->second);
  mHandles.erase(it);
}

void KeyFrameDatabase::clear() {
  std::unique_lock<std::mutex> lock(mMutex);
  if (mpDb && osh_bow_db_clear(mpDb) != OSH_OK) std::fprintf(stderr, "KeyFrameDatabase::clear: %s\n", osh_last_error());
  mKeyFrames.clear();
  mHandles.clear();
}

void KeyFrameDatabase::clearMap(Map* pMap) {
  std::unique_lock<std::mutex> lock(mMutex);
  for (auto it = mKeyFrames.begin(); it != mKeyFrames.end();) {
    KeyFrame* pKFi = it->second;
    if (pMap == pKFi->GetMap()) {   // the keyframe's map now, as :87
      if (osh_bow_db_erase(mpDb, it->first) != OSH_OK) std::fprintf(stderr, "KeyFrameDatabase::clearMap: %s\n", osh_last_error());
      mHandles.erase(pKFi);
      it = mKeyFrames.erase(it);
    } else {
      ++it;
    }
  }
}

void KeyFrameDatabase::SetORBVocabulary(ORBVocabulary* pORBVoc) {
  std::unique_lock<std::mutex> lock(mMutex);
  mpVoc = pORBVoc;
  mbRefused = false;
  if (mpVoc && mpVoc->getScoringType() != DBoW2::L1_NORM) {
    std::fprintf(stderr, "KeyFrameDatabase: the vocabulary's scoring type %d is not L1_NORM; the database stays empty\n", (int)mpVoc->getScoringType());
    mbRefused = true;
  }
  if (mpDb) { osh_bow_db_destroy(mpDb); mpDb = nullptr; }   // the word count is the database's
  mKeyFrames.clear();
  mHandles.clear();
}

bool KeyFrameDatabase::Query(const DBoW2::BowVector& bow, const std::vector<uint64_t>& excluded, std::vector<Listed>& rows) {
  rows.clear();
  osh_orb_ctx* ctx = HostMatcherContext();
  if (!ctx) return false;
  std::vector<int32_t> id;
  std::vector<double> value;
  flatten(bow, id, value);
  const size_t cap = mKeyFrames.size();
  std::vector<uint64_t> handle(cap);
  std::vector<int32_t> common(cap), first(cap);
  std::vector<uint8_t> scored(cap);
  std::vector<double> score(cap);
  int32_t n = 0;
  osh_bow_db_query q{};
  q.n = (int32_t)id.size(); q.word_id = id.data(); q.value = value.data();
  q.n_excluded = (int32_t)excluded.size(); q.excluded = excluded.data();
  osh_bow_db_result r{};
  r.capacity = (int32_t)cap; r.n_rows = &n;
  r.handle = handle.data(); r.common = common.data(); r.first_word = first.data(); r.scored = scored.data(); r.score = score.data();
  if (osh_orb_bow_db_query(ctx, mpDb, 1, &q, &r) != OSH_OK) {
    std::fprintf(stderr, "KeyFrameDatabase: %s\n", osh_last_error());
    return false;
  }
  std::vector<int> order(n);
  for (int k = 0; k < n; ++k) order[k] = k;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return first[a] != first[b] ? first[a] < first[b] : handle[a] < handle[b]; });
  rows.reserve(n);
  for (int k : order) rows.push_back({mKeyFrames.at(handle[k]), common[k], scored[k] != 0, score[k]});
  return true;
}

void KeyFrameDatabase::DetectNBestCandidates(KeyFrame* pKF, std::vector<KeyFrame*>& vpLoopCand, std::vector<KeyFrame*>& vpMergeCand, int nNumCandidates) {
  std::list<KeyFrame*> lKFsSharingWords;
  std::set<KeyFrame*> spConnectedKF;
  std::list<std::pair<float, KeyFrame*>> lScoreAndMatch;

  // Search all keyframes that share a word with current frame
  {
    std::unique_lock<std::mutex> lock(mMutex);
    if (!Usable("DetectNBestCandidates")) return;
    spConnectedKF = pKF->GetConnectedKeyFrames();
    // what the walk keeps out of lKFsSharingWords: the connected keyframes and those whose marker already equals the query id
    std::vector<uint64_t> excluded;
    for (const auto& e : mKeyFrames)
      if (e.second->mnPlaceRecognitionQuery == pKF->mnId || spConnectedKF.count(e.second)) excluded.push_back(e.first);
    std::vector<Listed> rows;
    if (!Query(pKF->mBowVec, excluded, rows)) return;
    for (const Listed& row : rows) {   // :623-633 with the row's count in place of one visit per shared word
      KeyFrame* pKFi = row.pKF;
      if (pKFi->mnPlaceRecognitionQuery != pKF->mnId) {
        pKFi->mnPlaceRecognitionWords = 0;
        if (!spConnectedKF.count(pKFi)) {
          pKFi->mnPlaceRecognitionQuery = pKF->mnId;
          lKFsSharingWords.push_back(pKFi);
          pKFi->mnPlaceRecognitionWords = row.words;
        } else {
          pKFi->mnPlaceRecognitionWords = 1;   // reset at every visit, then counted once
        }
      } else {
        pKFi->mnPlaceRecognitionWords += row.words;
      }
      // Compute similarity score (:655-666): the device scored the listed rows with more than minCommonWords words
      if (row.scored) {
        const float si = (float)row.score;
        pKFi->mPlaceRecognitionScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
  }
  if (lKFsSharingWords.empty()) return;
  if (lScoreAndMatch.empty()) return;

  std::list<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
  float bestAccScore = 0;

  // Lets now accumulate score by covisibility
  for (auto it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
    KeyFrame* pKFi = it->second;
    std::vector<KeyFrame*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);

    float bestScore = it->first;
    float accScore = bestScore;
    KeyFrame* pBestKF = pKFi;
    for (auto vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
      KeyFrame* pKF2 = *vit;
      if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;

      accScore += pKF2->mPlaceRecognitionScore;
      if (pKF2->mPlaceRecognitionScore > bestScore) {
        pBestKF = pKF2;
        bestScore = pKF2->mPlaceRecognitionScore;
      }
    }
    lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
    if (accScore > bestAccScore) bestAccScore = accScore;
  }

  lAccScoreAndMatch.sort(compFirst);

  vpLoopCand.reserve(nNumCandidates);
  vpMergeCand.reserve(nNumCandidates);
  std::set<KeyFrame*> spAlreadyAddedKF;
  size_t i = 0;
  const size_t nMax = (size_t)nNumCandidates;   // the reference compares size() with the int
  auto it = lAccScoreAndMatch.begin();
  while (i < lAccScoreAndMatch.size() && (vpLoopCand.size() < nMax || vpMergeCand.size() < nMax)) {
    KeyFrame* pKFi = it->second;
    if (pKFi->isBad()) { i++; it++; continue; }   // the intended deviation

    if (!spAlreadyAddedKF.count(pKFi)) {
      if (pKF->GetMap() == pKFi->GetMap() && vpLoopCand.size() < nMax) {
        vpLoopCand.push_back(pKFi);
      } else if (pKF->GetMap() != pKFi->GetMap() && vpMergeCand.size() < nMax && !pKFi->GetMap()->IsBad()) {
        vpMergeCand.push_back(pKFi);
      }
      spAlreadyAddedKF.insert(pKFi);
    }
    i++;
    it++;
  }
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F, Map* pMap) {
  std::list<KeyFrame*> lKFsSharingWords;
  std::list<std::pair<float, KeyFrame*>> lScoreAndMatch;

  // Search all keyframes that share a word with current frame
  {
    std::unique_lock<std::mutex> lock(mMutex);
    if (!Usable("DetectRelocalizationCandidates")) return std::vector<KeyFrame*>();
    std::vector<uint64_t> excluded;
    for (const auto& e : mKeyFrames)
      if (e.second->mnRelocQuery == F->mnId) excluded.push_back(e.first);
    std::vector<Listed> rows;
    if (!Query(F->mBowVec, excluded, rows)) return std::vector<KeyFrame*>();
    for (const Listed& row : rows) {   // :748-754
      KeyFrame* pKFi = row.pKF;
      if (pKFi->mnRelocQuery != F->mnId) {
        pKFi->mnRelocWords = 0;
        pKFi->mnRelocQuery = F->mnId;
        lKFsSharingWords.push_back(pKFi);
      }
      pKFi->mnRelocWords += row.words;
      if (row.scored) {                // :776-787
        const float si = (float)row.score;
        pKFi->mRelocScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
  }
  if (lKFsSharingWords.empty()) return std::vector<KeyFrame*>();
  if (lScoreAndMatch.empty()) return std::vector<KeyFrame*>();

  std::list<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
  float bestAccScore = 0;

  // Lets now accumulate score by covisibility
  for (auto it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
    KeyFrame* pKFi = it->second;
    std::vector<KeyFrame*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);

    float bestScore = it->first;
    float accScore = bestScore;
    KeyFrame* pBestKF = pKFi;
    for (auto vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
      KeyFrame* pKF2 = *vit;
      if (pKF2->mnRelocQuery != F->mnId) continue;

      accScore += pKF2->mRelocScore;
      if (pKF2->mRelocScore > bestScore) {
        pBestKF = pKF2;
        bestScore = pKF2->mRelocScore;
      }
    }
    lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
    if (accScore > bestAccScore) bestAccScore = accScore;
  }

  // Return all those keyframes with a score higher than 0.75*bestScore
  float minScoreToRetain = 0.75f * bestAccScore;
  std::set<KeyFrame*> spAlreadyAddedKF;
  std::vector<KeyFrame*> vpRelocCandidates;
  vpRelocCandidates.reserve(lAccScoreAndMatch.size());
  for (auto it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
    const float& si = it->first;
    if (si > minScoreToRetain) {
      KeyFrame* pKFi = it->second;
      if (pKFi->GetMap() != pMap) continue;
      if (!spAlreadyAddedKF.count(pKFi)) {
        vpRelocCandidates.push_back(pKFi);
        spAlreadyAddedKF.insert(pKFi);
      }
    }
  }

  return vpRelocCandidates;
}

}  // namespace ORB_SLAM3
