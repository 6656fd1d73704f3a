// overlay of tests/cvstub/Frame.h (placed in front of it on the include path, same include guard) for adapter/pnp/PnPsolver.cc: what the
// constructor of PnPsolver reads (include/Frame.h: mvKeysUn, mvLevelSigma2, mvpMapPoints, fx fy cx cy)
#ifndef CVSTUB_FRAME_H
#define CVSTUB_FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class Frame
{
public:
    Frame() : N(0) {}

    static float fx, fy, cx, cy;
    int N;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
};
}
#endif
