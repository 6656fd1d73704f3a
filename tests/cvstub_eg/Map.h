// stand-in for include/Map.h for adapter/essential/OptimizeEssentialGraph.cc: GetAllKeyFrames, GetAllMapPoints, mMutexMapUpdate
#ifndef CVSTUB_MAP_H
#define CVSTUB_MAP_H
#include <mutex>
#include <vector>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint;
class Map
{
public:
    std::vector<KeyFrame *> GetAllKeyFrames() { return mspKeyFrames; }
    std::vector<MapPoint *> GetAllMapPoints() { return mspMapPoints; }
    std::mutex mMutexMapUpdate;
    std::vector<KeyFrame *> mspKeyFrames;      // std::set, protected, in the reference: the stand-in keeps the order it is given
    std::vector<MapPoint *> mspMapPoints;
};
}
#endif
