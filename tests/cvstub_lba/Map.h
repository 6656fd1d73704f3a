// stand-in for include/Map.h: the one member Optimizer::LocalBundleAdjustment uses (include/Map.h:66: std::mutex mMutexMapUpdate)
#ifndef CVSTUB_MAP_H
#define CVSTUB_MAP_H
#include <mutex>
namespace ORB_SLAM2 {
class Map
{
public:
    std::mutex mMutexMapUpdate;
};
}
#endif
