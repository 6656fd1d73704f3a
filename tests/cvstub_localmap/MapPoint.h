// overlay of tests/cvstub/MapPoint.h (placed in front of it on the include path, same include guard): everything the stand-in declares,
// plus what adapter/localmap/LocalMapPoints.cc touches -- mnLastFrameSeen, IncreaseVisible (include/MapPoint.h:96, :68), mMutexPos, and the
// accessor the adaptor defines (one declaration added to include/MapPoint.h)
#ifndef CVSTUB_MAPPOINT_H
#define CVSTUB_MAPPOINT_H
#include <map>
#include <mutex>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class Frame;
class MapPoint
{
public:
    explicit MapPoint(bool bad = false) { init(); mbBad = bad; }
    MapPoint(const MapPoint &o) { copy(o); }
    MapPoint &operator=(const MapPoint &o) { copy(o); return *this; }

    bool isBad() { return mbBad; }                       // include/MapPoint.h: bool isBad();
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    int Observations() { return nObs; }
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    int PredictScale(const float &currentDist, KeyFrame *pKF);
    int PredictScale(const float &currentDist, Frame *pF);
    void AddObservation(KeyFrame *pKF, size_t idx) { if (!mObservations.count(pKF)) { mObservations[pKF] = idx; nObs++; } }
    void Replace(MapPoint *pMP) { mbBad = true; mpReplaced = pMP; }
    void ComputeDistinctiveDescriptors();               // defined by adapter/MapPoint_distinctive.cc
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    void GetFrustumRecord(float *geom8, unsigned char *desc32);   // defined by adapter/localmap/LocalMapPoints.cc

    // the variables Tracking::SearchLocalPoints / Frame::isInFrustum leave for SearchByProjection (include/MapPoint.h:89-95)
    float mTrackProjX, mTrackProjY, mTrackProjXR;
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos;
    long unsigned int mnLastFrameSeen;

    // protected in the reference
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    std::map<KeyFrame *, size_t> mObservations;
    float mfMinDistance, mfMaxDistance;
    MapPoint *mpReplaced;
    int nObs, mnVisible;
    bool mbBad;
    std::mutex mMutexFeatures, mMutexPos;

private:
    void init()
    {
        mTrackProjX = mTrackProjY = mTrackProjXR = 0.f; mbTrackInView = false; mnTrackScaleLevel = 0; mTrackViewCos = 0.f;
        mnLastFrameSeen = 0; mfMinDistance = 0.f; mfMaxDistance = 1e9f; mpReplaced = NULL; nObs = 0; mnVisible = 1; mbBad = false;
    }
    void copy(const MapPoint &o)
    {
        mTrackProjX = o.mTrackProjX; mTrackProjY = o.mTrackProjY; mTrackProjXR = o.mTrackProjXR; mbTrackInView = o.mbTrackInView;
        mnTrackScaleLevel = o.mnTrackScaleLevel; mTrackViewCos = o.mTrackViewCos; mnLastFrameSeen = o.mnLastFrameSeen;
        mWorldPos = o.mWorldPos; mNormalVector = o.mNormalVector;
        mDescriptor = o.mDescriptor; mObservations = o.mObservations; mfMinDistance = o.mfMinDistance; mfMaxDistance = o.mfMaxDistance;
        mpReplaced = o.mpReplaced; nObs = o.nObs; mnVisible = o.mnVisible; mbBad = o.mbBad;
    }
};
}
#endif
