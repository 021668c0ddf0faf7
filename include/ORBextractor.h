/* ORBextractor.h -- the one member of ORB_SLAM3::ORBextractor that Frame::ComputeStereoMatches reads (reference
 * include/ORBextractor.h:83).  Minimal test double; extraction itself is not part of this repository. */
#ifndef ORBEXTRACTOR_H
#define ORBEXTRACTOR_H
#include <vector>
#include "orbslam3_compat.h"
namespace ORB_SLAM3 {
class ORBextractor {
 public:
  std::vector<cv::Mat> mvImagePyramid;
};
}  // namespace ORB_SLAM3
#endif
