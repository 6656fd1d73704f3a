// stand-in for include/KeyFrame.h (tests/cvstub_eg comes first on the include path) for adapter/essential/OptimizeEssentialGraph.cc: the
// members Optimizer::OptimizeEssentialGraph uses -- mnId, isBad, GetPose, SetPose, GetParent, hasChild, GetLoopEdges,
// GetCovisiblesByWeight, GetWeight.  The stand-in's own: SetPose counts its calls and those made without the map's lock held.
#ifndef CVSTUB_KEYFRAME_H
#define CVSTUB_KEYFRAME_H
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame
{
public:
    KeyFrame() : mnId(0), mbBad(false), mpParent(NULL), set_pose_calls(0), unlocked_calls(0) {}
    bool isBad() { return mbBad; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_)
    {
        Tcw = Tcw_.clone(); set_pose_calls++;
        if (watch && watch->try_lock()) { watch->unlock(); unlocked_calls++; }
    }
    KeyFrame *GetParent() { return mpParent; }
    bool hasChild(KeyFrame *pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame *> GetLoopEdges() { return mspLoopEdges; }
    // src/KeyFrame.cc:188-203: the keyframes of mvpOrderedConnectedKeyFrames (weights descending) whose weight is at least w
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &w)
    {
        std::vector<KeyFrame *> out;
        for (size_t i = 0; i < ordered.size(); i++)
            if (ordered[i].second >= w) out.push_back(ordered[i].first);
        return out;
    }
    int GetWeight(KeyFrame *pKF)
    {
        for (size_t i = 0; i < ordered.size(); i++)
            if (ordered[i].first == pKF) return ordered[i].second;
        return 0;
    }

    long unsigned int mnId;
    bool mbBad;                                                  // protected in the reference
    cv::Mat Tcw;                                                 // protected in the reference
    KeyFrame *mpParent;                                          // protected in the reference
    std::set<KeyFrame *> mspChildrens, mspLoopEdges;             // protected in the reference
    std::vector<std::pair<KeyFrame *, int> > ordered;            // mvpOrderedConnectedKeyFrames with mvOrderedWeights, weights descending
    int set_pose_calls, unlocked_calls;                          // the stand-in's own
    static std::mutex *watch;                                    // the map's mMutexMapUpdate, defined by the driver
};
}
#endif
