// Stand-ins for the reference's KeyFrame, MapPoint, Map, Frame and LocalMapping, for adapter/mapgraph/MapGraph.cc and its driver
// (tests/adapter_mapgraph_driver.cc): only the members that the observation bookkeeping touches, with the mutators of include/KeyFrame.h and
// include/MapPoint.h doing what the reference's do to mvpMapPoints / mObservations / nObs / mbBad and firing the hooks that
// INTEGRATION.md section 3o lists.  g_hooks switches the hooks off for the copy of the map that the plain host loops work on.
#ifndef CVSTUB_GRAPH_STUB_H
#define CVSTUB_GRAPH_STUB_H
#include <stddef.h>
#include <map>
#include <set>
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapGraph.h"

namespace ORB_SLAM2 {

extern bool g_hooks;
inline orbx_adapter::MapGraph &G() { return orbx_adapter::MapGraph::instance(); }

class MapPoint;
class Map;

class KeyFrame
{
public:
    KeyFrame(long unsigned int id, const std::vector<int> &octave, const std::vector<float> &uRight, const std::vector<float> &depth, float thDepth)
        : mnId(id), N((int)octave.size()), mvKeysUn(octave.size()), mvuRight(uRight), mvDepth(depth), mThDepth(thDepth), mvpMapPoints(octave.size(), (MapPoint *)NULL),
          mbNotErase(false), mbToBeErased(false), mbBad(false)
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

    long unsigned int mnId;
    const int N;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    float mThDepth;

    std::vector<MapPoint *> mvpMapPoints;                        // protected in the reference
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;        // protected in the reference
    bool mbNotErase, mbToBeErased, mbBad;                        // protected in the reference
};

class MapPoint
{
public:
    explicit MapPoint(long unsigned int id) : mnId(id), nObs(0), mbBad(false), mpReplaced(NULL) {}
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

class Frame
{
public:
    Frame() : N(0) {}
    int N;
    std::vector<MapPoint *> mvpMapPoints;
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
