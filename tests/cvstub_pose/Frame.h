// overlay of tests/cvstub/Frame.h (placed in front of it on the include path, same include guard) for adapter/pose/PoseOptimization.cc:
// what Optimizer::PoseOptimization reads and writes (include/Frame.h: N, mvKeysUn, mvuRight, mvpMapPoints, mvbOutlier, mvInvLevelSigma2,
// fx fy cx cy, mbf, mTcw, SetPose).  SetPose counts its calls: with fewer than 3 correspondences the reference never calls it.
#ifndef CVSTUB_FRAME_H
#define CVSTUB_FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class Frame
{
public:
    Frame() : mbf(0), N(0), set_pose_calls(0) {}
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); set_pose_calls++; }   // src/Frame.cc:294-298 (UpdatePoseMatrices is not needed here)

    static float fx, fy, cx, cy;
    float mbf;
    int N;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvInvLevelSigma2;
    cv::Mat mTcw;
    int set_pose_calls;    // the stand-in's own
};
}
#endif
