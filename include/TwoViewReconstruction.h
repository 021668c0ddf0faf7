/* TwoViewReconstruction.h -- ORB_SLAM3::TwoViewReconstruction with the reference's constructor and Reconstruct
 * (reference include/TwoViewReconstruction.h:38-43); csrc/host/TwoViewReconstruction.cc runs it in one osh_orb_two_view_reconstruct
 * call.  The private helpers of the reference (FindHomography .. DecomposeE) are statements of csrc/two_view.h there. */
#ifndef TwoViewReconstruction_H
#define TwoViewReconstruction_H
#include <utility>
#include <vector>
#include "orbslam3_compat.h"
namespace ORB_SLAM3 {
class TwoViewReconstruction {
  typedef std::pair<int, int> Match;

 public:
  // Fix the reference frame
  TwoViewReconstruction(const Eigen::Matrix3f& k, float sigma = 1.0, int iterations = 200);

  // Computes a fundamental matrix and a homography, selects a model and tries to recover the motion and the structure from motion
  bool Reconstruct(const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2, const std::vector<int>& vMatches12,
                   Sophus::SE3f& T21, std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated);

  // Not in the reference: what the last Reconstruct did, for the caller that wants to know why it returned false.
  int mnLastStatus = -1;          // OSH_TWOVIEW_* of include/orbslam3_hip.h
  bool mbLastOnDevice = false;    // false: the host build of csrc/two_view.h answered (limits exceeded, or a device error)
  const std::vector<std::vector<size_t> >& GetSets() const { return mvSets; }

 private:
  std::vector<Match> mvMatches12;   // Current Matches from Reference to Current (mvbMatched1 is written and never read: not kept)
  Eigen::Matrix3f mK;               // Calibration
  float mSigma, mSigma2;            // Standard Deviation and Variance
  int mMaxIterations;               // Ransac max iterations
  std::vector<std::vector<size_t> > mvSets;   // Ransac sets
};
}  // namespace ORB_SLAM3
#endif
