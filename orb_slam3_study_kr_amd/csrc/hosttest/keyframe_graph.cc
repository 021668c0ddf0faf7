// keyframe_graph.cc -- bodies of the stand-in KeyFrame's covisibility accessors used by Optimizer::OptimizeEssentialGraph.
#include <algorithm>
#include <vector>

#include "KeyFrame.h"

namespace ORB_SLAM3 {

// src/KeyFrame.cc:253-273: mvOrderedWeights is descending; upper_bound with weightComp (a > b) finds the first weight < w
std::vector<KeyFrame*> KeyFrame::GetCovisiblesByWeight(const int& w) {
  if (mvpOrderedConnectedKeyFrames.empty()) return std::vector<KeyFrame*>();
  auto it = std::upper_bound(mvOrderedWeights.begin(), mvOrderedWeights.end(), w, [](int a, int b) { return a > b; });
  if (it == mvOrderedWeights.end() && mvOrderedWeights.back() < w) return std::vector<KeyFrame*>();
  const int n = (int)(it - mvOrderedWeights.begin());
  return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
}

// src/KeyFrame.cc:275-282
int KeyFrame::GetWeight(KeyFrame* pKF) {
  const auto it = mConnectedKeyFrameWeights.find(pKF);
  return it != mConnectedKeyFrameWeights.end() ? it->second : 0;
}

}  // namespace ORB_SLAM3
