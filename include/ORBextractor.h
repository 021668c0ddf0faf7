/* ORBextractor.h -- the members of ORB_SLAM3::ORBextractor that Frame::ComputeStereoMatches reads (mvImagePyramid, reference
 * include/ORBextractor.h:83) and that ORBextractor::operator() and ORBextractor::ComputeKeyPointsOctTree (csrc/host/ORBextractor.cc)
 * need.  Minimal test double: the constructor (with a generated sampling table of its own) and DistributeOctTree live in
 * csrc/hosttest/orbextractor.cc; ComputePyramid (osh_orb_pyramid_build) and the blur and the descriptors of operator()
 * (osh_orb_describe) run on the device. */
#ifndef ORBEXTRACTOR_H
#define ORBEXTRACTOR_H
#include <vector>
#include "orbslam3_compat.h"
#include "RectifyMap.h"
namespace ORB_SLAM3 {
class ORBextractor {
 public:
  ORBextractor() {}
  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST);
  /* the reference's signature (include/ORBextractor.h:56); the mask is ignored there too */
  int operator()(cv::InputArray _image, cv::InputArray _mask, std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors,
                 std::vector<int>& vLappingArea);
  std::vector<cv::Mat> mvImagePyramid;

  /* protected in the reference; public here so that the test wrappers can call it */
  void ComputePyramid(cv::Mat image);
  void ComputeKeyPointsOctTree(std::vector<std::vector<cv::KeyPoint> >& allKeypoints);
  std::vector<cv::KeyPoint> DistributeOctTree(const std::vector<cv::KeyPoint>& vToDistributeKeys, const int& minX, const int& maxX,
                                              const int& minY, const int& maxY, const int& nFeatures, const int& level);

  /* ADD THIS MEMBER to the reference's class: DistributeOctTree with the same arguments and the same result, as one
   * osh_orb_octree_distribute call (csrc/orb_octree_device.hip).  Beyond the call's limits, without a context or on a device error
   * the same statements run on the host (osh::octree_distribute_host of csrc/orb_octree.h) after a message on stderr */
  std::vector<cv::KeyPoint> DistributeOctTreeDevice(const std::vector<cv::KeyPoint>& vToDistributeKeys, const int& minX, const int& maxX,
                                                    const int& minY, const int& maxY, const int& nFeatures, const int& level);

  /* ADD THIS MEMBER too: operator() of several extractors as ONE osh_orb_extract call (csrc/orb_extract_device.hip), for example
   * the left and the right extractor of a stereo frame: image i goes through extractor i, vKeypoints[i] / vDescriptors[i] /
   * vMonoIndex[i] are what operator() would leave in _keypoints / _descriptors and return (-1 for an empty image), with
   * vLappingAreas[i] as its vLappingArea.  The candidates stay on the device between the detector and the descriptors, and the
   * quadtree is the rule of include/orbslam3_hip.h, not DistributeOctTree.  Every extractor's mnPyramidToken names its levels on
   * the device; mvImagePyramid is filled as ComputePyramid fills it when bKeepPyramid is set and left with empty levels when not */
  static void ExtractBatch(const std::vector<ORBextractor*>& vpExtractors, const std::vector<cv::Mat>& vImages,
                           std::vector<std::vector<cv::KeyPoint> >& vKeypoints, std::vector<cv::Mat>& vDescriptors,
                           const std::vector<std::vector<int> >& vLappingAreas, std::vector<int>& vMonoIndex, bool bKeepPyramid = true);

  /* ADD THIS MEMBER too: ExtractBatch on the camera images as they arrive, as ONE osh_orb_extract_raw call
   * (csrc/orb_prepare_device.hip): vRawImages[i] (CV_8UC1, CV_8UC3 or CV_8UC4) is remapped with vPrep[i].pMap or resized to
   * vPrep[i].newRows x newCols on the device, turned grey with vPrep[i].bRGB, and extracted as ExtractBatch extracts the result, so
   * that the cv::remap / cv::resize of System::Track* and the cvtColor of Tracking::GrabImage* are not run.  Everything else is
   * ExtractBatch's.  *pvGray (may be null) receives the prepared grey images, what Tracking keeps as mImGray */
  static void ExtractBatchRaw(const std::vector<ORBextractor*>& vpExtractors, const std::vector<cv::Mat>& vRawImages,
                              const std::vector<ImagePrep>& vPrep, std::vector<std::vector<cv::KeyPoint> >& vKeypoints,
                              std::vector<cv::Mat>& vDescriptors, const std::vector<std::vector<int> >& vLappingAreas,
                              std::vector<int>& vMonoIndex, bool bKeepPyramid = true, std::vector<cv::Mat>* pvGray = nullptr);
  /* ADD THIS TYPE too: the stereo match that Frame::ExtractAndMatchStereo asks ExtractBatchFrom to run behind the extraction of
   * a left and a right image (osh_orb_extract_stereo, csrc/stereo_device.hip).  bOk: the call ran and both results fit; vuRight
   * and vDepth then hold one entry per left keypoint, in the order of vKeypoints[0] */
  struct StereoMatch {
    float bf = 0, b = 0;
    std::vector<float> vuRight, vDepth;
    bool bOk = false;
  };
  /* ADD THIS MEMBER too: the body of the two (pvPrep null: ExtractBatch).  pStereo (may be null): the call has exactly two
   * extractors with an image each, the left one first, and runs as ONE osh_orb_extract_stereo */
  static void ExtractBatchFrom(const char* who, const std::vector<ORBextractor*>& vpExtractors, const std::vector<cv::Mat>& vImages,
                               const std::vector<ImagePrep>* pvPrep, std::vector<std::vector<cv::KeyPoint> >& vKeypoints,
                               std::vector<cv::Mat>& vDescriptors, const std::vector<std::vector<int> >& vLappingAreas,
                               std::vector<int>& vMonoIndex, bool bKeepPyramid, std::vector<cv::Mat>* pvGray, StereoMatch* pStereo = nullptr);

  std::vector<cv::Point> pattern;   /* the 512 sampling points, filled by the constructor */

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

  /* ADD THIS MEMBER to the reference's class: the token of the pyramid the last ComputeKeyPointsOctTree left on the device
   * (0: none), which operator() hands to osh_orb_describe */
  uint64_t mnPyramidToken = 0;
  /* ADD THIS MEMBER too: the token of the pyramid the last ComputePyramid built on the device (0: none).  The next
   * ComputeKeyPointsOctTree consumes it: while it is valid the detector reads the resident levels, not mvImagePyramid */
  uint64_t mnBuiltPyramidToken = 0;

  /* test double only: every DistributeOctTree call of the last ComputeKeyPointsOctTree, as it was made */
  struct DistributeCall {
    std::vector<cv::KeyPoint> keys;
    int minX, maxX, minY, maxY, nFeatures, level;
  };
  std::vector<DistributeCall> mvDistributeCalls;
};
}  // namespace ORB_SLAM3
#endif
