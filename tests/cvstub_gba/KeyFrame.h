// overlay of tests/cvstub_lba/KeyFrame.h (placed in front of it on the include path, same include guard) for adapter/ba/BundleAdjustment.cc:
// the members Optimizer::BundleAdjustment uses (include/KeyFrame.h: mnId, isBad, GetPose, SetPose, mvKeysUn, mvuRight, mvInvLevelSigma2,
// fx fy cx cy mbf, and the loop-closing results mTcwGBA, mnBAGlobalForKF).  SetPose counts its calls.
#ifndef CVSTUB_KEYFRAME_H
#define CVSTUB_KEYFRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class KeyFrame
{
public:
    KeyFrame() : mnId(0), mnBAGlobalForKF(0), fx(0), fy(0), cx(0), cy(0), mbf(0), mbBad(false), set_pose_calls(0) {}
    bool isBad() { return mbBad; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); set_pose_calls++; }

    long unsigned int mnId;
    cv::Mat mTcwGBA;
    long unsigned int mnBAGlobalForKF;
    float fx, fy, cx, cy, mbf;
    std::vector<float> mvInvLevelSigma2;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;

    bool mbBad;                                                  // protected in the reference
    cv::Mat Tcw;                                                 // protected in the reference
    int set_pose_calls;                                          // the stand-in's own
};
}
#endif
