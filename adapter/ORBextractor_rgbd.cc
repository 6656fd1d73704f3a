// adapter/ORBextractor_rgbd.cc -- ORBextractor::ExtractRGBD: the RGB-D constructor's ExtractORB + UndistortKeyPoints + ComputeStereoFromRGBD
// (reference src/Frame.cc:145-154, :470-515, :754-774) with Tracking::GrabImageRGBD's depth convertTo (src/Tracking.cc:232-233) folded in,
// as ONE orbx_extract_rgbd call.  INTEGRATION.md shows the Frame / Tracking swap.
#include "ORBextractor.h"

#include <stdexcept>

namespace ORB_SLAM2
{

void ORBextractor::ExtractRGBD(const cv::Mat &imGray, const cv::Mat &imDepth, float depthScale, const cv::Mat &K, const cv::Mat &distCoef,
                               float bf, std::vector<cv::KeyPoint> &keys, std::vector<cv::KeyPoint> &keysUn, cv::Mat &descriptors,
                               std::vector<float> &uRight, std::vector<float> &depth)
{
    assert(imGray.type() == CV_8UC1 && imDepth.rows == imGray.rows && imDepth.cols == imGray.cols);
    orbx_rgbd_params p;
    if (imDepth.type() == CV_16U)                    // raw depth (the TUM PNGs): Tracking always converts it (:232)
        p.depth_type = ORBX_DEPTH_U16;
    else if (imDepth.type() == CV_32F)
        p.depth_type = ORBX_DEPTH_F32;
    else
        throw std::runtime_error("ExtractRGBD: depth must be CV_16U or CV_32F");
    p.depth_scale = depthScale;                      // Tracking::mDepthMapFactor
    p.bf = bf;
    p.fx = K.at<float>(0, 0); p.fy = K.at<float>(1, 1); p.cx = K.at<float>(0, 2); p.cy = K.at<float>(1, 2);
    p.ndist = distCoef.rows * distCoef.cols;         // 4 or 5 (Tracking.cc:80-96)
    for (int i = 0; i < 5; i++)
        p.dist_coef[i] = i < p.ndist ? distCoef.at<float>(i) : 0.0f;
    const int cap = orbx_max_keypoints(mH, imGray.cols, imGray.rows);
    if (cap < 0)
        throw std::runtime_error(orbx_last_error());
    keys.resize(cap);
    std::vector<float> xy(2 * (size_t)cap);
    cv::Mat desc(cap, 32, CV_8U);
    uRight.assign(cap, -1.0f);
    depth.assign(cap, -1.0f);
    int n = 0;
    // the depth map's own row step: a continuous Mat or a view into a larger one
    if (orbx_extract_rgbd(mH, imGray.data, imGray.cols, imGray.rows, imGray.step, 1, 1, imDepth.data, imDepth.step, &p,
                          reinterpret_cast<orbx_keypoint *>(&keys[0]), desc.data, cap, &n, &xy[0], &uRight[0], &depth[0]) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
    keys.resize(n);
    uRight.resize(n);
    depth.resize(n);
    keysUn = keys;                                   // src/Frame.cc:472-476 / :508-514: a copy whose positions are replaced
    for (int i = 0; i < n; i++) {
        keysUn[i].pt.x = xy[2 * i];
        keysUn[i].pt.y = xy[2 * i + 1];
    }
    if (n == 0)
        descriptors.release();
    else
        desc.rowRange(0, n).copyTo(descriptors);
}

} // namespace ORB_SLAM2
