/* MLPnPsolver.h -- ORB_SLAM3::MLPnPsolver with the reference's constructor, SetRansacParameters and iterate
 * (reference include/MLPnPsolver.h:62-77); csrc/host/MLPnPsolver.cc runs every iterate in one osh_orb_mlpnp_solve call.  The private
 * helpers of the reference (computePose, CheckInliers, Refine, mlpnp_gn ..) are statements of csrc/mlpnp.h there. */
#ifndef MLPNPSOLVER_H
#define MLPNPSOLVER_H
#include <array>
#include <cstdint>
#include <deque>
#include <vector>
#include "Frame.h"
#include "MapPoint.h"
#include "orbslam3_compat.h"
namespace ORB_SLAM3 {
class MLPnPsolver {
 public:
  MLPnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches);
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4,
                           float th2 = 5.991);
  // One device call: up to max(mRansacMaxIts - mnIterations, nIterations) minimal sets, as the reference's loop condition allows
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Eigen::Matrix4f& Tout);

  // Not in the reference: iterate of every solver (the candidate keyframes of Tracking::Relocalization) in one device call.  Entry k
  // of every output is what solvers[k]->iterate(nIterations, ..) returns and leaves; iterate is the batch of one.
  static void IterateBatch(const std::vector<MLPnPsolver*>& solvers, int nIterations, std::vector<bool>& vbFound, std::vector<bool>& vbNoMore,
                           std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers, std::vector<Eigen::Matrix4f>& vTout);

  // Not in the reference: what one round of iterate runs and what it came back with (csrc/host/MLPnPsolver.cc states the replay)
  struct Round {
    std::vector<int32_t> sets;   // [iterations * 6]: queued sets first, then newly drawn ones
    int iterations = 0;
    bool skip = false;           // N < mRansacMinInliers: no work, bNoMore
  };
  struct Outcome {
    int first_hit = -1, hit_record = -1, hit_count = 0, best_iteration = -1, best_count = 0, best_refine_ok = 0;
    double hit_pose[12] = {0}, best_pose[12] = {0};
    std::vector<uint32_t> hit_mask, best_mask;   // OSH_MLPNP_MASK_WORDS(N) words each
  };
  Round Prepare(int nIterations);
  bool Replay(const Round& round, const Outcome& o, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Eigen::Matrix4f& Tout);
  bool mbLastOnDevice = false;   // false: the host build of csrc/mlpnp.h answered (limits exceeded, no context, or a device error)
  int GetIterations() const { return mnIterations; }
  int GetBestInliers() const { return mnBestInliers; }
  int GetMinInliers() const { return mRansacMinInliers; }
  int GetMaxIterations() const { return mRansacMaxIts; }
  int GetN() const { return N; }
  size_t GetQueuedSets() const { return mvQueuedSets.size(); }

 private:
  std::vector<MapPoint*> mvpMapPointMatches;
  std::vector<cv::Point2f> mvP2D;             // 2D Points
  std::vector<std::array<double, 3> > mvBearingVecs;
  std::vector<float> mvSigma2;
  std::vector<std::array<double, 3> > mvP3Dw;   // 3D Points
  std::vector<size_t> mvKeyPointIndices;      // Index in Frame
  int mnIterations = 0;                       // Current Ransac State
  std::vector<bool> mvbBestInliers;
  int mnBestInliers = 0;
  Eigen::Matrix4f mBestTcw;
  Eigen::Matrix4f mRefinedTcw;                // Refined: of the current best, kept while it stays the best
  std::vector<bool> mvbRefinedInliers;
  int mnRefinedInliers = 0;
  bool mbBestRefineOk = false;                // whether Refine of the current best succeeds
  int N = 0;                                  // Number of Correspondences
  std::vector<size_t> mvAllIndices;           // Indices for random selection [0 .. N-1]
  double mRansacProb = 0.99;
  int mRansacMinInliers = 8, mRansacMaxIts = 300;
  float mRansacEpsilon = 0.4f;
  int mRansacMinSet = 6;
  std::vector<float> mvMaxError;              // Max square error associated with scale level
  GeometricCamera* mpCamera = nullptr;
  std::deque<std::array<int32_t, 6> > mvQueuedSets;   // drawn for an earlier call and not consumed by its early return
};
}  // namespace ORB_SLAM3
#endif
