// Stand-ins for the reference's KeyFrame, MapPoint, Map, Frame and LocalMapping, for adapter/mappoint/MapPointRefresh.cc, adapter/mapgraph/MapGraph.cc
// and their driver (tests/adapter_refresh_driver.cc): the stand-ins of tests/cvstub_graph (the observation bookkeeping with its hooks,
// INTEGRATION.md section 3o) and, on top, what the two refresh functions touch: the camera centre, descriptors and scale table of a
// keyframe; mWorldPos, mpRefKF, mNormalVector, mfMinDistance, mfMaxDistance and mDescriptor of a map point, with
// MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors doing what src/MapPoint.cc:371-420 and :266-340 do, on the
// cv::Mat arithmetic of tests/cvstub, the two setters that INTEGRATION.md section 3p adds, and what adapter/localmap/LocalMapPoints.cc
// touches of a map point (the Frame it searches is tests/cvstub_refresh/Frame.h).  g_hooks switches the hooks off for a
// point that the graph is not to know.
#ifndef CVSTUB_REFRESH_STUB_H
#define CVSTUB_REFRESH_STUB_H
#include <stddef.h>
#include <map>
#include <limits.h>
#include <algorithm>
#include <mutex>
#include <set>
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapGraph.h"

namespace ORB_SLAM2 {

extern bool g_hooks;
inline orbx_adapter::MapGraph &G() { return orbx_adapter::MapGraph::instance(); }

class MapPoint;
class Map;
class Frame;

class KeyFrame
{
public:
    KeyFrame(long unsigned int id, const std::vector<int> &octave, const std::vector<float> &uRight, const std::vector<float> &depth, float thDepth)
        : mnId(id), N((int)octave.size()), mvKeysUn(octave.size()), mvuRight(uRight), mvDepth(depth), mThDepth(thDepth), mvpMapPoints(octave.size(), (MapPoint *)NULL),
          mbNotErase(false), mbToBeErased(false), mbBad(false), mnScaleLevels(0), Ow(3, 1, CV_32F)
    {
        for (size_t i = 0; i < octave.size(); i++) mvKeysUn[i].octave = octave[i];
        if (g_hooks) G().OnNewKeyFrame(this);
    }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { if (g_hooks) G().OnSetMatch(this, idx, pMP); mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { if (g_hooks) G().OnSetMatch(this, idx, NULL); mvpMapPoints[idx] = NULL; }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { if (g_hooks) G().OnSetMatch(this, idx, pMP); mvpMapPoints[idx] = pMP; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    void SetNotErase() { mbNotErase = true; }
    bool GetNotErase() { return mbNotErase; }
    bool isBad() { return mbBad; }
    inline void SetBadFlag();
    cv::Mat GetCameraCenter() { return Ow.clone(); }

    long unsigned int mnId;
    const int N;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    float mThDepth;

    std::vector<MapPoint *> mvpMapPoints;                        // protected in the reference
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;        // protected in the reference
    bool mbNotErase, mbToBeErased, mbBad;                        // protected in the reference

    cv::Mat mDescriptors;                                        // N x 32, CV_8U
    std::vector<float> mvScaleFactors;
    int mnScaleLevels;
    cv::Mat Ow;                                                  // protected in the reference
};

class MapPoint
{
public:
    explicit MapPoint(long unsigned int id) : mnId(id), nObs(0), mbBad(false), mpReplaced(NULL), mWorldPos(3, 1, CV_32F), mpRefKF(NULL), mfMinDistance(0), mfMaxDistance(0),
                                              mnLastFrameSeen(0), mnVisible(1) {}
    // what adapter/localmap/LocalMapPoints.cc touches (as tests/cvstub_localmap/MapPoint.h)
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    void GetFrustumRecord(float *geom8, unsigned char *desc32);   // defined by adapter/localmap/LocalMapPoints.cc
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    inline void UpdateNormalAndDepth();
    inline void ComputeDistinctiveDescriptors();
    // what orbx_adapter::RefreshMapPoints stores (the reference takes mMutexPos / mMutexFeatures here)
    void SetNormalAndDepth(const cv::Mat &normal, float fMinDistance, float fMaxDistance) { mNormalVector = normal.clone(); mfMinDistance = fMinDistance; mfMaxDistance = fMaxDistance; }
    void SetDescriptor(const cv::Mat &descriptor) { mDescriptor = descriptor.clone(); }
    inline void AddObservation(KeyFrame *pKF, size_t idx);
    inline void EraseObservation(KeyFrame *pKF);
    inline void SetBadFlag();
    inline void Replace(MapPoint *pMP);
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }

    long unsigned int mnId;
    std::map<KeyFrame *, size_t> mObservations;                  // protected in the reference
    int nObs;
    bool mbBad;
    MapPoint *mpReplaced;
    cv::Mat mWorldPos;                                           // protected in the reference, as everything below
    KeyFrame *mpRefKF;
    cv::Mat mNormalVector, mDescriptor;
    float mfMinDistance, mfMaxDistance;
    long unsigned int mnLastFrameSeen;
    int mnVisible;
    std::mutex mMutexFeatures, mMutexPos;
};

class Map
{
public:
    void clear()
    {
        if (g_hooks) G().OnMapClear();
        for (std::set<MapPoint *>::iterator it = mspMapPoints.begin(); it != mspMapPoints.end(); ++it) delete *it;
        for (std::set<KeyFrame *>::iterator it = mspKeyFrames.begin(); it != mspKeyFrames.end(); ++it) delete *it;
        mspMapPoints.clear(); mspKeyFrames.clear();
    }
    std::set<MapPoint *> mspMapPoints;
    std::set<KeyFrame *> mspKeyFrames;
};

class LocalMapping
{
public:
    LocalMapping(bool bMonocular) : mbMonocular(bMonocular), mpCurrentKeyFrame(NULL) {}
    void KeyFrameCulling();                                      // defined by adapter/mapgraph/MapGraph.cc
    bool mbMonocular;
    KeyFrame *mpCurrentKeyFrame;
};

// ---- the mutators (src/MapPoint.cc:106-232, src/KeyFrame.cc:489-507): what they do to the two views, nothing else

inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx)
{
    if (g_hooks) G().OnAddObservation(this, pKF, idx);
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs += pKF->mvuRight[idx] >= 0 ? 2 : 1;
}

inline void MapPoint::EraseObservation(KeyFrame *pKF)
{
    if (g_hooks) G().OnEraseObservation(this, pKF);
    bool bBad = false;
    if (mObservations.count(pKF)) {
        const size_t idx = mObservations[pKF];
        nObs -= pKF->mvuRight[idx] >= 0 ? 2 : 1;
        mObservations.erase(pKF);
        if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
}

inline void MapPoint::SetBadFlag()
{
    if (g_hooks) G().OnPointBad(this);
    mbBad = true;
    std::map<KeyFrame *, size_t> obs;
    obs.swap(mObservations);
    for (std::map<KeyFrame *, size_t>::iterator mit = obs.begin(); mit != obs.end(); ++mit) mit->first->EraseMapPointMatch(mit->second);
}

inline void MapPoint::Replace(MapPoint *pMP)
{
    if (pMP->mnId == mnId) return;
    if (g_hooks) G().OnPointBad(this);
    std::map<KeyFrame *, size_t> obs;
    obs.swap(mObservations);
    mbBad = true;
    mpReplaced = pMP;
    for (std::map<KeyFrame *, size_t>::iterator mit = obs.begin(); mit != obs.end(); ++mit) {
        KeyFrame *pKF = mit->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF, mit->second);
        } else
            pKF->EraseMapPointMatch(mit->second);
    }
}

// ---- the two functions that orbx_adapter::RefreshMapPoints replaces: what src/MapPoint.cc:371-420 and :266-340 do

inline int DescriptorDistance(const cv::Mat &a, const cv::Mat &b)      // ORBmatcher::DescriptorDistance: the bits that differ
{
    int dist = 0;
    for (int i = 0; i < 32; i++) dist += __builtin_popcount((unsigned)(a.ptr<uchar>()[i] ^ b.ptr<uchar>()[i]));
    return dist;
}

inline void MapPoint::UpdateNormalAndDepth()
{
    if (mbBad) return;
    std::map<KeyFrame *, size_t> observations = mObservations;
    KeyFrame *pRefKF = mpRefKF;
    const cv::Mat Pos = mWorldPos.clone();
    if (observations.empty()) return;
    cv::Mat normal(3, 1, CV_32F);                                // zeros
    int n = 0;
    for (std::map<KeyFrame *, size_t>::iterator mit = observations.begin(); mit != observations.end(); ++mit) {
        const cv::Mat Owi = mit->first->GetCameraCenter();
        const cv::Mat normali = mWorldPos - Owi;
        normal = normal + normali / cv::norm(normali);
        n++;
    }
    const cv::Mat PC = Pos - pRefKF->GetCameraCenter();
    const float dist = (float)cv::norm(PC);
    const int level = pRefKF->mvKeysUn[observations[pRefKF]].octave;     // operator[] on the copy: a missing key reads index 0
    const float levelScaleFactor = pRefKF->mvScaleFactors[level];
    const int nLevels = pRefKF->mnScaleLevels;
    mfMaxDistance = dist * levelScaleFactor;
    mfMinDistance = mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
    mNormalVector = normal / n;
}

inline void MapPoint::ComputeDistinctiveDescriptors()
{
    if (mbBad) return;
    const std::map<KeyFrame *, size_t> observations = mObservations;
    if (observations.empty()) return;
    std::vector<cv::Mat> vDescriptors;
    for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit)
        if (!mit->first->isBad()) vDescriptors.push_back(mit->first->mDescriptors.row((int)mit->second));
    if (vDescriptors.empty()) return;
    const size_t N = vDescriptors.size();
    std::vector<int> Distances(N * N, 0);
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) Distances[i * N + j] = Distances[j * N + i] = DescriptorDistance(vDescriptors[i], vDescriptors[j]);
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(Distances.begin() + (long)(i * N), Distances.begin() + (long)((i + 1) * N));
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (N - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    mDescriptor = vDescriptors[BestIdx].clone();
}

inline void KeyFrame::SetBadFlag()
{
    if (mnId == 0) return;
    if (mbNotErase) { mbToBeErased = true; return; }
    if (g_hooks) G().OnKeyFrameBad(this);
    for (size_t i = 0; i < mvpMapPoints.size(); i++)
        if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
    mbBad = true;
}

}
#endif
