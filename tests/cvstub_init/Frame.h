// overlay of tests/cvstub/Frame.h (placed in front of it on the include path, same include guard) for adapter/init/Initializer.cc: what
// Initializer reads of a Frame (include/Frame.h: mK, mvKeysUn), and the cv::Point3f of its interface, which tests/cvstub does not define
#ifndef CVSTUB_FRAME_H
#define CVSTUB_FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
namespace cv {
template <typename T> struct Point3_ {
    T x, y, z;
    Point3_() : x(0), y(0), z(0) {}
    Point3_(T _x, T _y, T _z) : x(_x), y(_y), z(_z) {}
};
typedef Point3_<float> Point3f;
}
namespace ORB_SLAM2 {
class Frame
{
public:
    Frame() {}

    cv::Mat mK;
    std::vector<cv::KeyPoint> mvKeysUn;
};
}
#endif
