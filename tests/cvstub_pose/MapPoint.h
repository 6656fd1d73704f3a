// overlay of tests/cvstub/MapPoint.h (placed in front of it on the include path, same include guard) for adapter/pose/PoseOptimization.cc:
// the world position and the lock the reference's gather holds (include/MapPoint.h:47, :81: GetWorldPos, static std::mutex mGlobalMutex)
#ifndef CVSTUB_MAPPOINT_H
#define CVSTUB_MAPPOINT_H
#include <mutex>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class MapPoint
{
public:
    MapPoint() : mWorldPos(3, 1, CV_32F) {}
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    static std::mutex mGlobalMutex;
    cv::Mat mWorldPos;     // protected in the reference
};
}
#endif
