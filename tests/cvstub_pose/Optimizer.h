// stand-in for include/Optimizer.h: the one declaration adapter/pose/PoseOptimization.cc defines, as the reference declares it
// (include/Optimizer.h:53: `int static PoseOptimization(Frame* pFrame);`).  The reference's header also includes Map.h, KeyFrame.h, LoopClosing.h
// and g2o, which the adaptor does not touch.
#ifndef CVSTUB_OPTIMIZER_H
#define CVSTUB_OPTIMIZER_H
#include "Frame.h"
#include "MapPoint.h"
namespace ORB_SLAM2 {
class Optimizer
{
public:
    int static PoseOptimization(Frame *pFrame);
};
}
#endif
