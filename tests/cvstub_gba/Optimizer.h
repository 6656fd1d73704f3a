// overlay of tests/cvstub_lba/Optimizer.h (same include guard): the two declarations adapter/ba/BundleAdjustment.cc defines, as the
// reference declares them (include/Optimizer.h:40-44), default arguments included
#ifndef CVSTUB_OPTIMIZER_H
#define CVSTUB_OPTIMIZER_H
#include <cstddef>
#include <vector>
#include "Map.h"
#include "MapPoint.h"
#include "KeyFrame.h"
namespace ORB_SLAM2 {
class Optimizer
{
public:
    static void BundleAdjustment(const std::vector<KeyFrame *> &vpKF, const std::vector<MapPoint *> &vpMP, int nIterations = 5,
                                 bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);
    static void GlobalBundleAdjustemnt(Map *pMap, int nIterations = 5, bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                                       const bool bRobust = true);
};
}
#endif
