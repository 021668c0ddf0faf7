// kfdb.cc -- the osh_host_kfdb_* and osh_host_bowdb_* wrappers of include/orbslam3_hip_host.h: a plain single-thread C++ restatement
// of KeyFrameDatabase (src/KeyFrameDatabase.cc:32-98, 604-845) with the real std::vector<std::list<KeyFrame*>> inverted file (the CPU
// baseline of profiles/kfdb_timing.py and the yardstick of the host layer), the real ORB_SLAM3::KeyFrameDatabase driven through the
// same scripts of operations, both on stand-in graphs built from flat arrays, and a replay of add / erase / clear through the
// bookkeeping of osh_bow_db (csrc/bowdb_book.h) that needs no device.  Test library only.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <list>
#include <memory>
#include <set>
#include <vector>

#include "../bowdb_book.h"
#include "Frame.h"
#include "KeyFrame.h"
#include "KeyFrameDatabase.h"
#include "Map.h"
#include "ORBVocabulary.h"
#include "orbslam3_hip_host.h"

using namespace ORB_SLAM3;

struct osh_host_bow_vocab { ORBVocabulary voc; };   // as csrc/hosttest/bow.cc

namespace {

// L1Scoring::score (ScoringObject.cpp:23-68)
double l1_score(const DBoW2::BowVector& v1, const DBoW2::BowVector& v2) {
#pragma clang fp contract(off)
  auto v1_it = v1.begin(), v2_it = v2.begin();
  double score = 0;
  while (v1_it != v1.end() && v2_it != v2.end()) {
    const double vi = v1_it->second, wi = v2_it->second;
    if (v1_it->first == v2_it->first) {
      score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
      ++v1_it; ++v2_it;
    } else if (v1_it->first < v2_it->first) {
      v1_it = v1.lower_bound(v2_it->first);
    } else {
      v2_it = v2.lower_bound(v1_it->first);
    }
  }
  return -score / 2.0;
}

bool compFirst(const std::pair<float, KeyFrame*>& a, const std::pair<float, KeyFrame*>& b) { return a.first > b.first; }

// The reference's class with its inverted file, one thread, no mutex
struct Restated {
  std::vector<std::list<KeyFrame*>> mvInvertedFile;
  explicit Restated(size_t n_words) : mvInvertedFile(n_words) {}

  void add(KeyFrame* pKF) {
    for (auto vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) mvInvertedFile[vit->first].push_back(pKF);
  }
  void erase(KeyFrame* pKF) {
    for (auto vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) {
      std::list<KeyFrame*>& lKFs = mvInvertedFile[vit->first];
      for (auto lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++)
        if (pKF == *lit) { lKFs.erase(lit); break; }
    }
  }
  void clear() { const size_t n = mvInvertedFile.size(); mvInvertedFile.clear(); mvInvertedFile.resize(n); }
  void clearMap(Map* pMap) {
    for (auto& lKFs : mvInvertedFile)
      for (auto lit = lKFs.begin(); lit != lKFs.end();) {
        if (pMap == (*lit)->GetMap()) lit = lKFs.erase(lit); else ++lit;
      }
  }

  void DetectNBestCandidates(KeyFrame* pKF, std::vector<KeyFrame*>& vpLoopCand, std::vector<KeyFrame*>& vpMergeCand, int nNumCandidates) {
    std::list<KeyFrame*> lKFsSharingWords;
    std::set<KeyFrame*> spConnectedKF = pKF->GetConnectedKeyFrames();
    for (auto vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) {
      std::list<KeyFrame*>& lKFs = mvInvertedFile[vit->first];
      for (auto lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
        KeyFrame* pKFi = *lit;
        if (pKFi->mnPlaceRecognitionQuery != pKF->mnId) {
          pKFi->mnPlaceRecognitionWords = 0;
          if (!spConnectedKF.count(pKFi)) {
            pKFi->mnPlaceRecognitionQuery = pKF->mnId;
            lKFsSharingWords.push_back(pKFi);
          }
        }
        pKFi->mnPlaceRecognitionWords++;
      }
    }
    if (lKFsSharingWords.empty()) return;

    int maxCommonWords = 0;
    for (KeyFrame* k : lKFsSharingWords)
      if (k->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = k->mnPlaceRecognitionWords;
    int minCommonWords = maxCommonWords * 0.8f;

    std::list<std::pair<float, KeyFrame*>> lScoreAndMatch;
    for (KeyFrame* pKFi : lKFsSharingWords)
      if (pKFi->mnPlaceRecognitionWords > minCommonWords) {
        float si = l1_score(pKF->mBowVec, pKFi->mBowVec);
        pKFi->mPlaceRecognitionScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    if (lScoreAndMatch.empty()) return;

    std::list<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
    float bestAccScore = 0;
    for (auto it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KeyFrame* pKFi = it->second;
      std::vector<KeyFrame*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KeyFrame* pBestKF = pKFi;
      for (KeyFrame* pKF2 : vpNeighs) {
        if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;
        accScore += pKF2->mPlaceRecognitionScore;
        if (pKF2->mPlaceRecognitionScore > bestScore) { pBestKF = pKF2; bestScore = pKF2->mPlaceRecognitionScore; }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    lAccScoreAndMatch.sort(compFirst);

    std::set<KeyFrame*> spAlreadyAddedKF;
    size_t i = 0;
    const size_t nMax = (size_t)nNumCandidates;
    auto it = lAccScoreAndMatch.begin();
    while (i < lAccScoreAndMatch.size() && (vpLoopCand.size() < nMax || vpMergeCand.size() < nMax)) {
      KeyFrame* pKFi = it->second;
      if (pKFi->isBad()) { i++; it++; continue; }   // :712 of the reference never advances; skipped here as in the class
      if (!spAlreadyAddedKF.count(pKFi)) {
        if (pKF->GetMap() == pKFi->GetMap() && vpLoopCand.size() < nMax) vpLoopCand.push_back(pKFi);
        else if (pKF->GetMap() != pKFi->GetMap() && vpMergeCand.size() < nMax && !pKFi->GetMap()->IsBad()) vpMergeCand.push_back(pKFi);
        spAlreadyAddedKF.insert(pKFi);
      }
      i++;
      it++;
    }
  }

  std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F, Map* pMap) {
    std::list<KeyFrame*> lKFsSharingWords;
    for (auto vit = F->mBowVec.begin(), vend = F->mBowVec.end(); vit != vend; vit++) {
      std::list<KeyFrame*>& lKFs = mvInvertedFile[vit->first];
      for (auto lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
        KeyFrame* pKFi = *lit;
        if (pKFi->mnRelocQuery != F->mnId) {
          pKFi->mnRelocWords = 0;
          pKFi->mnRelocQuery = F->mnId;
          lKFsSharingWords.push_back(pKFi);
        }
        pKFi->mnRelocWords++;
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KeyFrame*>();

    int maxCommonWords = 0;
    for (KeyFrame* k : lKFsSharingWords)
      if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;
    int minCommonWords = maxCommonWords * 0.8f;

    std::list<std::pair<float, KeyFrame*>> lScoreAndMatch;
    for (KeyFrame* pKFi : lKFsSharingWords)
      if (pKFi->mnRelocWords > minCommonWords) {
        float si = l1_score(F->mBowVec, pKFi->mBowVec);
        pKFi->mRelocScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    if (lScoreAndMatch.empty()) return std::vector<KeyFrame*>();

    std::list<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
    float bestAccScore = 0;
    for (auto it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KeyFrame* pKFi = it->second;
      std::vector<KeyFrame*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KeyFrame* pBestKF = pKFi;
      for (KeyFrame* pKF2 : vpNeighs) {
        if (pKF2->mnRelocQuery != F->mnId) continue;
        accScore += pKF2->mRelocScore;
        if (pKF2->mRelocScore > bestScore) { pBestKF = pKF2; bestScore = pKF2->mRelocScore; }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }

    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KeyFrame*> spAlreadyAddedKF;
    std::vector<KeyFrame*> vpRelocCandidates;
    for (auto it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
      const float& si = it->first;
      if (si > minScoreToRetain) {
        KeyFrame* pKFi = it->second;
        if (pKFi->GetMap() != pMap) continue;
        if (!spAlreadyAddedKF.count(pKFi)) { vpRelocCandidates.push_back(pKFi); spAlreadyAddedKF.insert(pKFi); }
      }
    }
    return vpRelocCandidates;
  }
};

// The stand-in graph of an osh_host_kfdb_graph
struct Graph {
  std::vector<std::unique_ptr<Map>> maps;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<Frame>> frames;
  std::map<KeyFrame*, int> index;

  bool build(const osh_host_kfdb_graph* g) {
    if (!g || g->n_kf < 0 || g->n_maps < 1 || g->n_frames < 0 || g->n_words < 1) return false;
    for (int m = 0; m < g->n_maps; ++m) { maps.emplace_back(new Map()); maps.back()->mbBad = g->map_bad && g->map_bad[m]; }
    for (int k = 0; k < g->n_kf; ++k) {
      if (g->kf_map[k] < 0 || g->kf_map[k] >= g->n_maps) return false;
      kfs.emplace_back(new KeyFrame((long unsigned int)g->kf_id[k], maps[g->kf_map[k]].get()));
      KeyFrame* kf = kfs.back().get();
      kf->mbBad = g->kf_bad && g->kf_bad[k];
      for (int e = g->bow_start[k]; e < g->bow_start[k + 1]; ++e) {
        if (g->bow_word[e] < 0 || g->bow_word[e] >= g->n_words) return false;
        kf->mBowVec[(unsigned)g->bow_word[e]] = g->bow_value[e];
      }
      index[kf] = k;
    }
    for (int k = 0; k < g->n_kf; ++k) {
      for (int e = g->cov_start[k]; e < g->cov_start[k + 1]; ++e) {
        if (g->cov[e] < 0 || g->cov[e] >= g->n_kf) return false;
        kfs[k]->mvpOrderedConnectedKeyFrames.push_back(kfs[g->cov[e]].get());
      }
      for (int e = g->con_start[k]; e < g->con_start[k + 1]; ++e) {
        if (g->con[e] < 0 || g->con[e] >= g->n_kf) return false;
        kfs[k]->mConnectedKeyFrameWeights[kfs[g->con[e]].get()] = 1;
      }
    }
    for (int f = 0; f < g->n_frames; ++f) {
      frames.emplace_back(new Frame());
      frames.back()->mnId = (long unsigned int)g->fr_id[f];
      for (int e = g->fr_start[f]; e < g->fr_start[f + 1]; ++e) {
        if (g->fr_word[e] < 0 || g->fr_word[e] >= g->n_words) return false;
        frames.back()->mBowVec[(unsigned)g->fr_word[e]] = g->fr_value[e];
      }
    }
    return true;
  }
};

// Runs the script on `db` (Restated or the real class); the outputs of query q go to slot q of `out`.  Returns the number of queries,
// -1 for a bad operation
template <class Db>
int run_script(Db& db, Graph& G, const osh_host_kfdb_graph* g, int n_ops, const int32_t* ops, const osh_host_kfdb_out* out, double* ms) {
  int q = 0;
  double total = 0;
  const size_t n_kf = G.kfs.size();
  for (int o = 0; o < n_ops; ++o) {
    const int code = ops[3 * o], a = ops[3 * o + 1], b = ops[3 * o + 2];
    const bool kf_op = code == OSH_HOST_KFDB_ADD || code == OSH_HOST_KFDB_ERASE || code == OSH_HOST_KFDB_NBEST;
    if (kf_op && (a < 0 || a >= (int)n_kf)) return -1;
    if ((code == OSH_HOST_KFDB_CLEAR_MAP && (a < 0 || a >= g->n_maps)) || (code == OSH_HOST_KFDB_RELOC && (a < 0 || a >= g->n_frames || b < 0 || b >= g->n_maps))) return -1;
    std::vector<KeyFrame*> loop, merge;
    switch (code) {
      case OSH_HOST_KFDB_ADD: db.add(G.kfs[a].get()); continue;
      case OSH_HOST_KFDB_ERASE: db.erase(G.kfs[a].get()); continue;
      case OSH_HOST_KFDB_CLEAR_MAP: db.clearMap(G.maps[a].get()); continue;
      case OSH_HOST_KFDB_CLEAR: db.clear(); continue;
      case OSH_HOST_KFDB_NBEST: {
        const auto t0 = std::chrono::steady_clock::now();
        db.DetectNBestCandidates(G.kfs[a].get(), loop, merge, b);
        total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        break;
      }
      case OSH_HOST_KFDB_RELOC: {
        const auto t0 = std::chrono::steady_clock::now();
        loop = db.DetectRelocalizationCandidates(G.frames[a].get(), G.maps[b].get());
        total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        break;
      }
      default: return -1;
    }
    if (out) {
      if (out->n_loop) out->n_loop[q] = (int32_t)loop.size();
      if (out->n_merge) out->n_merge[q] = (int32_t)merge.size();
      for (size_t k = 0; k < loop.size() && out->loop; ++k) out->loop[(size_t)q * n_kf + k] = G.index.at(loop[k]);
      for (size_t k = 0; k < merge.size() && out->merge; ++k) out->merge[(size_t)q * n_kf + k] = G.index.at(merge[k]);
      for (size_t k = 0; k < n_kf; ++k) {
        const KeyFrame& kf = *G.kfs[k];
        if (out->marker) {
          int64_t* m = out->marker + ((size_t)q * n_kf + k) * 4;
          m[0] = (int64_t)kf.mnPlaceRecognitionQuery; m[1] = kf.mnPlaceRecognitionWords; m[2] = (int64_t)kf.mnRelocQuery; m[3] = kf.mnRelocWords;
        }
        if (out->score) {
          float* s = out->score + ((size_t)q * n_kf + k) * 2;
          s[0] = kf.mPlaceRecognitionScore; s[1] = kf.mRelocScore;
        }
      }
    }
    ++q;
  }
  if (ms) *ms = total;
  return q;
}

}  // namespace

extern "C" int osh_host_kfdb_restatement(const osh_host_kfdb_graph* g, int32_t n_ops, const int32_t* ops, const osh_host_kfdb_out* out, double* ms) {
  Graph G;
  if (n_ops < 0 || (n_ops && !ops) || !G.build(g)) return -1;
  Restated db((size_t)g->n_words);
  return run_script(db, G, g, n_ops, ops, out, ms);
}

extern "C" int osh_host_kfdb_run(osh_host_bow_vocab* voc, const osh_host_kfdb_graph* g, int32_t n_ops, const int32_t* ops, const osh_host_kfdb_out* out,
                                 double* ms) {
  Graph G;
  if (!voc || n_ops < 0 || (n_ops && !ops) || !G.build(g)) return -1;
  if ((int64_t)voc->voc.size() < g->n_words) return -2;   // the graph's words have to be words of the vocabulary
  KeyFrameDatabase db(voc->voc);
  return run_script(db, G, g, n_ops, ops, out, ms);
}

extern "C" int osh_host_bowdb_check_words(int32_t n, const int32_t* word_id, int64_t n_words) {
  int64_t at = 0;
  return osh::bowdb_check_words(n, word_id, n_words, &at);
}

extern "C" int osh_host_bowdb_book_replay(int32_t n_ops, const int64_t* ops, uint64_t* op_handle, int32_t max_rows, uint64_t* handle, int64_t* start,
                                          int32_t* len, uint8_t* alive, int64_t info[8]) {
  if (n_ops < 0 || (n_ops && !ops) || !info) return -1;
  osh::BowDbBook book;
  int64_t moved = 0;
  for (int o = 0; o < n_ops; ++o) {
    const int64_t code = ops[2 * o], arg = ops[2 * o + 1];
    if (op_handle) op_handle[o] = 0;
    if (code == 0) {          // add a row of arg entries
      if (arg < 0) return -1;
      for (const osh::BowDbMove& m : book.prepare((size_t)arg, 1).moves) moved += m.len;
      const int r = book.append((int32_t)arg);
      if (op_handle) op_handle[o] = book.handle[r];
    } else if (code == 1) {   // erase the handle arg
      if (book.find((uint64_t)arg) < 0) return -2;
      for (const osh::BowDbMove& m : book.prepare(0, 0).moves) moved += m.len;
      book.erase(book.find((uint64_t)arg));
    } else if (code == 2) {
      book.clear();
    } else {
      return -1;
    }
  }
  const int n = (int)book.row.size();
  if (n > max_rows) return -3;
  for (int r = 0; r < n; ++r) {
    if (handle) handle[r] = book.handle[r];
    if (start) start[r] = book.row[r].start;
    if (len) len[r] = book.row[r].len;
    if (alive) alive[r] = (uint8_t)book.row[r].alive;
  }
  info[0] = (int64_t)book.live_rows; info[1] = n; info[2] = (int64_t)book.entries; info[3] = (int64_t)book.entry_cap;
  info[4] = book.compactions; info[5] = book.reallocations; info[6] = (int64_t)book.row_cap; info[7] = moved;
  return n;
}
