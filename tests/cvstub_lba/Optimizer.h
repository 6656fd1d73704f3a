// stand-in for include/Optimizer.h: the one declaration adapter/lba/LocalBundleAdjustment.cc defines, as the reference declares it
// (include/Optimizer.h:52: `void static LocalBundleAdjustment(KeyFrame* pKF, bool *pbStopFlag, Map *pMap);`).  The reference's header also
// includes LoopClosing.h, Frame.h and g2o, which the adaptor does not touch.
#ifndef CVSTUB_OPTIMIZER_H
#define CVSTUB_OPTIMIZER_H
#include "Map.h"
#include "MapPoint.h"
#include "KeyFrame.h"
namespace ORB_SLAM2 {
class Optimizer
{
public:
    void static LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap);
};
}
#endif
