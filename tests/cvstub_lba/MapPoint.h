// overlay of tests/cvstub/MapPoint.h (placed in front of it on the include path, same include guard) for adapter/lba/LocalBundleAdjustment.cc:
// the members Optimizer::LocalBundleAdjustment uses (include/MapPoint.h: mnId, mnBALocalForKF, isBad, GetObservations, GetWorldPos,
// SetWorldPos, UpdateNormalAndDepth, EraseObservation).  The stand-in's own: update_calls / set_calls count, bad_on_read makes the point
// bad when its position is read (another thread's SetBadFlag between the gather and the final loops), and every erased pair goes to a log.
#ifndef CVSTUB_MAPPOINT_H
#define CVSTUB_MAPPOINT_H
#include <map>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint
{
public:
    MapPoint() : mnId(0), mnBALocalForKF(0), mWorldPos(3, 1, CV_32F), mbBad(false), bad_on_read(false), update_calls(0), set_calls(0) {}
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    cv::Mat GetWorldPos() { if (bad_on_read) mbBad = true; return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); set_calls++; }
    void UpdateNormalAndDepth() { update_calls++; }
    void EraseObservation(KeyFrame *pKF) { mObservations.erase(pKF); erase_log().push_back(std::make_pair(pKF, this)); }
    static std::vector<std::pair<KeyFrame *, MapPoint *> > &erase_log() { static std::vector<std::pair<KeyFrame *, MapPoint *> > v; return v; }

    long unsigned int mnId;
    long unsigned int mnBALocalForKF;
    cv::Mat mWorldPos;                                // protected in the reference
    std::map<KeyFrame *, size_t> mObservations;       // protected in the reference
    bool mbBad;                                       // protected in the reference
    bool bad_on_read;
    int update_calls, set_calls;
};
}
#endif
