// overlay of tests/cvstub/KeyFrame.h (placed in front of it on the include path, same include guard) for adapter/lba/LocalBundleAdjustment.cc:
// the members Optimizer::LocalBundleAdjustment uses (include/KeyFrame.h: mnId, mnBALocalForKF, mnBAFixedForKF, isBad,
// GetVectorCovisibleKeyFrames, GetMapPointMatches, GetPose, SetPose, EraseMapPointMatch, mvKeysUn, mvuRight, mvInvLevelSigma2, fx fy cx cy mbf).
// SetPose and EraseMapPointMatch count their calls.
#ifndef CVSTUB_KEYFRAME_H
#define CVSTUB_KEYFRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class KeyFrame
{
public:
    KeyFrame() : mnId(0), mnBALocalForKF(0), mnBAFixedForKF(0), fx(0), fy(0), cx(0), cy(0), mbf(0), mbBad(false), set_pose_calls(0), erase_calls(0) {}
    bool isBad() { return mbBad; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); set_pose_calls++; }
    void EraseMapPointMatch(MapPoint *pMP)
    {
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] == pMP) mvpMapPoints[i] = NULL;
        erase_calls++;
    }

    long unsigned int mnId;
    long unsigned int mnBALocalForKF, mnBAFixedForKF;
    float fx, fy, cx, cy, mbf;
    std::vector<float> mvInvLevelSigma2;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;

    bool mbBad;                                                  // protected in the reference
    std::vector<MapPoint *> mvpMapPoints;                        // protected in the reference
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;        // protected in the reference
    cv::Mat Tcw;                                                 // protected in the reference
    int set_pose_calls, erase_calls;                             // the stand-in's own
};
}
#endif
