// overlay of tests/cvstub/MapPoint.h (placed in front of it on the include path, same include guard): everything the stub declares, with a
// Replace that changes the SURVIVOR's descriptor, as the reference's does -- MapPoint::Replace moves the observations over and ends in
// pMP->ComputeDistinctiveDescriptors() (src/MapPoint.cc:190-229).  Here the change is a fixed function of the survivor's bytes: the first
// three bytes are inverted (the point still matches what it matched), or the first six when the last byte is odd (it no longer does).
// tests/adapter_kfframe_driver.cc uses it to show that orbx_adapter::FuseBatch searches such points again.
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
    int PredictScale(const float &currentDist, KeyFrame *pKF);     // src/MapPoint.cc:393-415; defined in tests/adapter_driver.cc
    int PredictScale(const float &currentDist, Frame *pF);
    void AddObservation(KeyFrame *pKF, size_t idx) { if (!mObservations.count(pKF)) { mObservations[pKF] = idx; nObs++; } }
    void Replace(MapPoint *pMP)
    {
        mbBad = true; mpReplaced = pMP;
        if (pMP->mDescriptor.empty()) return;
        cv::Mat d = pMP->mDescriptor.clone();
        const int nb = (d.data[31] & 1) ? 6 : 3;
        for (int b = 0; b < nb; b++) d.data[b] ^= 0xFF;
        pMP->mDescriptor = d;
    }
    void ComputeDistinctiveDescriptors();               // defined by adapter/MapPoint_distinctive.cc

    // the variables Tracking::SearchLocalPoints / Frame::isInFrustum leave for SearchByProjection (include/MapPoint.h:89-95)
    float mTrackProjX, mTrackProjY, mTrackProjXR;
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos;

    // protected in the reference
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    std::map<KeyFrame *, size_t> mObservations;
    float mfMinDistance, mfMaxDistance;
    MapPoint *mpReplaced;
    int nObs;
    bool mbBad;
    std::mutex mMutexFeatures;

private:
    void init()
    {
        mTrackProjX = mTrackProjY = mTrackProjXR = 0.f; mbTrackInView = false; mnTrackScaleLevel = 0; mTrackViewCos = 0.f;
        mfMinDistance = 0.f; mfMaxDistance = 1e9f; mpReplaced = NULL; nObs = 0; mbBad = false;
    }
    void copy(const MapPoint &o)
    {
        mTrackProjX = o.mTrackProjX; mTrackProjY = o.mTrackProjY; mTrackProjXR = o.mTrackProjXR; mbTrackInView = o.mbTrackInView;
        mnTrackScaleLevel = o.mnTrackScaleLevel; mTrackViewCos = o.mTrackViewCos; mWorldPos = o.mWorldPos; mNormalVector = o.mNormalVector;
        mDescriptor = o.mDescriptor; mObservations = o.mObservations; mfMinDistance = o.mfMinDistance; mfMaxDistance = o.mfMaxDistance;
        mpReplaced = o.mpReplaced; nObs = o.nObs; mbBad = o.mbBad;
    }
};
}
#endif
