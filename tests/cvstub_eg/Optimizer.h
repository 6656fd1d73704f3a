// stand-in for include/Optimizer.h: the one declaration adapter/essential/OptimizeEssentialGraph.cc defines, as the reference declares it
// (include/Optimizer.h:49-53, which is `using namespace std` through its includes)
#ifndef CVSTUB_OPTIMIZER_H
#define CVSTUB_OPTIMIZER_H
#include <map>
#include <set>
#include "Map.h"
#include "MapPoint.h"
#include "KeyFrame.h"
#include "LoopClosing.h"
namespace ORB_SLAM2 {
class Optimizer
{
public:
    void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                       const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections,
                                       const bool &bFixScale);
};
}
#endif
