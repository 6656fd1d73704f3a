// stand-in for include/MapPoint.h for adapter/essential/OptimizeEssentialGraph.cc: isBad, mnCorrectedByKF, mnCorrectedReference,
// GetReferenceKeyFrame, GetWorldPos, SetWorldPos, UpdateNormalAndDepth.  The stand-in's own: the two call counts.
#ifndef CVSTUB_MAPPOINT_H
#define CVSTUB_MAPPOINT_H
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint
{
public:
    MapPoint() : mnId(0), mnCorrectedByKF(0), mnCorrectedReference(0), mWorldPos(3, 1, CV_32F), mbBad(false), mpRefKF(NULL), update_calls(0), set_calls(0) {}
    bool isBad() { return mbBad; }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); set_calls++; }
    void UpdateNormalAndDepth() { update_calls++; }

    long unsigned int mnId;
    long unsigned int mnCorrectedByKF, mnCorrectedReference;
    cv::Mat mWorldPos;                                // protected in the reference
    bool mbBad;                                       // protected in the reference
    KeyFrame *mpRefKF;                                // protected in the reference
    int update_calls, set_calls;
};
}
#endif
