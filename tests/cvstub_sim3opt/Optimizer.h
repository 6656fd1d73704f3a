// stand-in for include/Optimizer.h: the one declaration adapter/sim3opt/OptimizeSim3.cc defines, as the reference declares it
// (include/Optimizer.h:56-57; tests/golden/reference_optimizesim3_interface.json holds it, tests/test_sim3opt_adapter.py compares).  The
// reference's header also includes Map.h, LoopClosing.h and Frame.h, which the adaptor does not touch.
#ifndef CVSTUB_OPTIMIZER_H
#define CVSTUB_OPTIMIZER_H
#include <vector>
#include "MapPoint.h"
#include "KeyFrame.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
namespace ORB_SLAM2 {
class Optimizer
{
public:
    static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint *> &vpMatches1,
                            g2o::Sim3 &g2oS12, const float th2, const bool bFixScale);
};
}
#endif
