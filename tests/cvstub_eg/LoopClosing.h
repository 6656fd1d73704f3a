// stand-in for include/LoopClosing.h: the one type Optimizer::OptimizeEssentialGraph takes from it (:49-50; the reference adds Eigen's
// aligned allocator, which the stand-in g2o::Sim3 does not need)
#ifndef CVSTUB_LOOPCLOSING_H
#define CVSTUB_LOOPCLOSING_H
#include <functional>
#include <map>
#include "KeyFrame.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
namespace ORB_SLAM2 {
class LoopClosing
{
public:
    typedef std::map<KeyFrame *, g2o::Sim3, std::less<KeyFrame *> > KeyFrameAndPose;
};
}
#endif
