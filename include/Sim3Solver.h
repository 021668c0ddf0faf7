/* Sim3Solver.h -- ORB_SLAM3::Sim3Solver with the reference's public interface (reference include/Sim3Solver.h:35-56);
 * csrc/host/Sim3Solver.cc runs all iterations between two SetRansacParameters in one osh_orb_sim3_ransac call and replays the kept
 * answer.  The private helpers of the reference (ComputeSim3, CheckInliers, Project ..) are statements of csrc/sim3_ransac.h there. */
#ifndef SIM3SOLVER_H
#define SIM3SOLVER_H
#include <cstdint>
#include <vector>
#include "CameraModels/GeometricCamera.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbslam3_compat.h"
struct osh_sim3r_problem;
namespace ORB_SLAM3 {
class Sim3Solver {
 public:
  Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true,
             std::vector<KeyFrame*> vpKeyFrameMatchedMP = std::vector<KeyFrame*>());
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);
  Eigen::Matrix4f find(std::vector<bool>& vbInliers12, int& nInliers);
  Eigen::Matrix4f iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);
  Eigen::Matrix4f iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge);
  Eigen::Matrix4f GetEstimatedTransformation() { return mBestT12; }
  Eigen::Matrix3f GetEstimatedRotation() { return mBestRotation; }
  Eigen::Vector3f GetEstimatedTranslation() { return mBestTranslation; }
  float GetEstimatedScale() { return mBestScale; }

  /* ADD THIS MEMBER to the reference's class: the five-argument iterate of every solver (the candidates of one
   * LoopClosing::DetectCommonRegionsFromBoW) with every pending device call made as one.  Entry k of every output is what
   * solvers[k]->iterate(nIterations, ..) returns and leaves; iterate is the batch of one. */
  static void IterateBatch(const std::vector<Sim3Solver*>& solvers, int nIterations, std::vector<bool>& vbNoMore,
                           std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers, std::vector<bool>& vbConverge,
                           std::vector<Eigen::Matrix4f>& vT12);

  // Not in the reference: what the one device call runs and what it came back with (csrc/host/Sim3Solver.cc states the replay)
  struct Round {
    std::vector<int32_t> sets;   // [iterations * 3], drawn as :172-186 draw them
    int iterations = 0;
    bool pending = false;        // sets were drawn: a device call is due and its answer is to be kept
  };
  struct Answer {
    int n_records = 0;
    std::vector<int32_t> record, record_count;   // [iterations]
    std::vector<float> record_T;                 // [iterations * 13]
    std::vector<uint32_t> record_mask;           // [iterations * OSH_SIM3R_MASK_WORDS(N)]
  };
  Round Prepare();                                // draws nothing while an answer is kept or when iterate would return at once
  void Keep(const Round& round, const Answer& a);
  void FillProblem(osh_sim3r_problem& p) const;   // everything of the device call but the sets
  Eigen::Matrix4f Replay(int nIterations, bool five, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge);
  bool mbLastOnDevice = false;   // false: the host build of csrc/sim3_ransac.h answered (limits exceeded, no context, or a device error)
  int GetIterations() const { return mnIterations; }
  int GetBestInliers() const { return mnBestInliers; }
  int GetMinInliers() const { return mRansacMinInliers; }
  int GetMaxIterations() const { return mRansacMaxIts; }
  int GetN() const { return N; }
  int GetN1() const { return mN1; }
  bool HasAnswer() const { return mbAnswer; }
  const std::vector<bool>& GetBestInlierFlags() const { return mvbBestInliers; }
  // the constructor's pack, as the device call receives it
  const std::vector<float>& GetX3Dc1() const { return mvX3Dc1; }
  const std::vector<float>& GetX3Dc2() const { return mvX3Dc2; }
  const std::vector<float>& GetP1im1() const { return mvP1im1; }
  const std::vector<float>& GetP2im2() const { return mvP2im2; }
  const std::vector<float>& GetMaxError1() const { return mvMaxError1; }
  const std::vector<float>& GetMaxError2() const { return mvMaxError2; }
  const std::vector<size_t>& GetIndices1() const { return mvnIndices1; }

 private:
  KeyFrame* mpKF1 = nullptr;
  KeyFrame* mpKF2 = nullptr;
  std::vector<float> mvX3Dc1, mvX3Dc2;          // [N * 3]
  std::vector<MapPoint*> mvpMapPoints1, mvpMapPoints2, mvpMatches12;
  std::vector<size_t> mvnIndices1;
  std::vector<size_t> mvnMaxError1, mvnMaxError2;   // size_t as in the reference (include/Sim3Solver.h:78-79): 9.210 * sigma2 truncated
  std::vector<float> mvMaxError1, mvMaxError2;      // (float) of them, what the comparison of CheckInliers converts to
  int N = 0, mN1 = 0;
  int mnIterations = 0;
  std::vector<bool> mvbBestInliers;
  int mnBestInliers = 0;
  Eigen::Matrix4f mBestT12;
  Eigen::Matrix3f mBestRotation;
  Eigen::Vector3f mBestTranslation;
  float mBestScale = 0;
  bool mbFixScale = true;
  std::vector<size_t> mvAllIndices;             // Indices for random selection
  std::vector<float> mvP1im1, mvP2im2;          // [N * 2] Projections
  double mRansacProb = 0.99;
  int mRansacMinInliers = 6, mRansacMaxIts = 300;
  GeometricCamera* pCamera1 = nullptr;
  GeometricCamera* pCamera2 = nullptr;
  // the kept answer of the device call: iteration mnAnswerBase + i of the solver is iteration i of the answer
  bool mbAnswer = false;
  int mnAnswerBase = 0, mnAnswerIterations = 0;
  Answer mAnswer;
  std::vector<int32_t> mvRecordOf;              // [answer iterations] the record ordinal of the iteration, -1: no record
};
}  // namespace ORB_SLAM3
#endif
