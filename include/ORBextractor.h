/* ORBextractor.h -- the members of ORB_SLAM3::ORBextractor that Frame::ComputeStereoMatches reads (mvImagePyramid, reference
 * include/ORBextractor.h:83) and that ORBextractor::ComputeKeyPointsOctTree (csrc/host/ORBextractor.cc) needs.  Minimal test double:
 * the constructor and DistributeOctTree live in csrc/hosttest/orbextractor.cc, and the pyramid, the blur and the descriptors
 * (ComputePyramid, operator()) are not part of this repository. */
#ifndef ORBEXTRACTOR_H
#define ORBEXTRACTOR_H
#include <vector>
#include "orbslam3_compat.h"
namespace ORB_SLAM3 {
class ORBextractor {
 public:
  ORBextractor() {}
  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST);
  std::vector<cv::Mat> mvImagePyramid;

  /* protected in the reference; public here so that the test wrappers can call it */
  void ComputeKeyPointsOctTree(std::vector<std::vector<cv::KeyPoint> >& allKeypoints);
  std::vector<cv::KeyPoint> DistributeOctTree(const std::vector<cv::KeyPoint>& vToDistributeKeys, const int& minX, const int& maxX,
                                              const int& minY, const int& maxY, const int& nFeatures, const int& level);

  int nfeatures = 0;
  double scaleFactor = 1.0;
  int nlevels = 0;
  int iniThFAST = 0;
  int minThFAST = 0;
  std::vector<int> mnFeaturesPerLevel;
  std::vector<float> mvScaleFactor;
  std::vector<float> mvInvScaleFactor;
  std::vector<float> mvLevelSigma2;
  std::vector<float> mvInvLevelSigma2;

  /* test double only: every DistributeOctTree call of the last ComputeKeyPointsOctTree, as it was made */
  struct DistributeCall {
    std::vector<cv::KeyPoint> keys;
    int minX, maxX, minY, maxY, nFeatures, level;
  };
  std::vector<DistributeCall> mvDistributeCalls;
};
}  // namespace ORB_SLAM3
#endif
