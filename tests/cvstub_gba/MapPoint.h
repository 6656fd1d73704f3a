// overlay of tests/cvstub_lba/MapPoint.h (placed in front of it on the include path, same include guard) for adapter/ba/BundleAdjustment.cc:
// the members Optimizer::BundleAdjustment uses (include/MapPoint.h: mnId, isBad, GetObservations, GetWorldPos, SetWorldPos,
// UpdateNormalAndDepth, and the loop-closing results mPosGBA, mnBAGlobalForKF).  The stand-in's own: update_calls / set_calls count,
// bad_on_read makes the point bad when its position is read (another thread's SetBadFlag between the gather and the recovery).
#ifndef CVSTUB_MAPPOINT_H
#define CVSTUB_MAPPOINT_H
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint
{
public:
    MapPoint() : mnId(0), mnBAGlobalForKF(0), mWorldPos(3, 1, CV_32F), mbBad(false), bad_on_read(false), update_calls(0), set_calls(0) {}
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    cv::Mat GetWorldPos() { if (bad_on_read) mbBad = true; return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); set_calls++; }
    void UpdateNormalAndDepth() { update_calls++; }

    long unsigned int mnId;
    cv::Mat mPosGBA;
    long unsigned int mnBAGlobalForKF;
    cv::Mat mWorldPos;                                // protected in the reference
    std::map<KeyFrame *, size_t> mObservations;       // protected in the reference
    bool mbBad;                                       // protected in the reference
    bool bad_on_read;
    int update_calls, set_calls;
};
}
#endif
