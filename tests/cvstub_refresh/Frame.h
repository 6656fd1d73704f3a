// overlay of tests/cvstub/Frame.h (placed in front of it on the include path, same include guard), as tests/cvstub_localmap/Frame.h: everything
// the stand-in declares, plus what adapter/localmap/LocalMapPoints.cc reads -- mRcw, mtcw, mOw (Frame::UpdatePoseMatrices,
// src/Frame.cc:300-306) and mnId; its map points are those of RefreshStub.h
#ifndef CVSTUB_FRAME_H
#define CVSTUB_FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
#include "ORBextractor.h"
#include <Thirdparty/DBoW2/DBoW2/BowVector.h>
#include <Thirdparty/DBoW2/DBoW2/FeatureVector.h>
namespace ORB_SLAM2 {
class Frame
{
public:
    Frame() : mpORBextractorLeft(NULL), mpORBextractorRight(NULL), mbf(0), mb(0), N(0), mnScaleLevels(0), mfLogScaleFactor(0), mnId(0) {}
    void ComputeStereoMatches();
    void ComputeBoW();              // defined by adapter/Frame_bow.cc
    void UndistortKeyPoints();      // defined by adapter/Frame_bow.cc
    void UpdatePoseMatrices()       // src/Frame.cc:300-306
    {
        mRcw = mTcw.rowRange(0, 3).colRange(0, 3);
        mtcw = mTcw.rowRange(0, 3).col(3);
        mOw = -mRcw.t() * mtcw;
    }

    ORBextractor *mpORBextractorLeft, *mpORBextractorRight;
    static float fx, fy, cx, cy;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    float mbf, mb;
    int N;
    int mnScaleLevels;
    float mfLogScaleFactor;
    long unsigned int mnId;
    std::vector<float> mvScaleFactors;
    std::vector<bool> mvbOutlier;
    cv::Mat mTcw, mK, mDistCoef;
    cv::Mat mRcw, mtcw, mOw;        // private in the reference (Frame::isInFrustum reads them)
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptors, mDescriptorsRight;
    std::vector<MapPoint *> mvpMapPoints;
};
}
#endif
