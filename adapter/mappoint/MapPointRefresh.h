// adapter/mappoint/MapPointRefresh.h -- the loops over map points behind the long steps of LocalMapping and LoopClosing, as one device call.
//
// After SearchInNeighbors, CreateNewMapPoints, the bundle adjustments and the essential-graph correction the reference loops over map
// points and calls MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:371-420) and MapPoint::ComputeDistinctiveDescriptors (:266-340).
// RefreshMapPoints runs both for a whole list in one orbx_mapgraph_refresh_points call on the resident observation graph
// (adapter/mapgraph/MapGraph.h), the resident keyframes and, when the process has one, the LocalMapPoints table, which is written in
// place; the MapPoint members are stored from what the call hands back.  Call sites: INTEGRATION.md section 3p.
//
// Additions to the reference:
//   include/MapPoint.h     void SetNormalAndDepth(const cv::Mat &normal, float fMinDistance, float fMaxDistance);   (under mMutexPos)
//                          void SetDescriptor(const cv::Mat &descriptor);                                            (under mMutexFeatures)
#ifndef ORBX_ADAPTER_MAPPOINTREFRESH_H
#define ORBX_ADAPTER_MAPPOINTREFRESH_H

#include <atomic>
#include <memory>
#include <vector>

#include <orbx.h>

namespace ORB_SLAM2
{
class KeyFrame;
class MapPoint;
}

namespace orbx_adapter
{

enum { REFRESH_GEOM = ORBX_REFRESH_GEOM, REFRESH_DESC = ORBX_REFRESH_DESC };

// What RefreshMapPoints asks of the rest of the adaptor.  The owners announce themselves when they come to life (KeyFrameFrames in
// ORBmatcher_batch.cc: frame_of; LocalMapPoints in localmap/LocalMapPoints.cc: table); an entry left NULL means that part is not linked in
// or not in use, and RefreshMapPoints does without it.  Header-only, so that a program links only what it uses; atomic, because the owner
// may come to life on one thread while another refreshes.
typedef std::shared_ptr<const orbx_frame> (*RefreshFrameOf)(ORB_SLAM2::KeyFrame *pKF);   // the registered resident frame, empty when none
// The process's map-point table, lent for one refresh.  begin() shuts the owner's searches out and hands over the handle -- or returns
// NULL, with nothing held, while there is no table.  Until end(): slot() is the slot a point holds (-1: none; nothing is handed out), and
// refreshed() tells the owner which halves of the record the device holds now (what & REFRESH_GEOM: geom8 = X Y Z min nx ny nz max;
// what & REFRESH_DESC: desc32), AFTER the point's members have been stored.  No search of the owner's runs between the device write, the
// members and the owner's bookkeeping, so it never sees two of them disagree.
struct RefreshTable {
    orbx_mappoints *(*begin)();
    int (*slot)(ORB_SLAM2::MapPoint *pMP);
    void (*refreshed)(ORB_SLAM2::MapPoint *pMP, int slot, int what, const float *geom8, const unsigned char *desc32);
    void (*end)();
};
struct RefreshHooks {
    std::atomic<RefreshFrameOf> frame_of;
    std::atomic<const RefreshTable *> table;
};
inline RefreshHooks &refresh_hooks()
{
    static RefreshHooks h;      // static storage: both start out NULL
    return h;
}

struct RefreshStats { int on_device, on_host, desc_on_host, abi_calls; };

// UpdateNormalAndDepth (what & REFRESH_GEOM) and ComputeDistinctiveDescriptors (what & REFRESH_DESC) of every point of the list (NULL
// entries are skipped, a point listed twice is taken once).  The entries of a row are taken in ascending keyframe SLOT (include/orbx.h), the
// reference's in KeyFrame* address order: equal wherever slots and addresses ascend together.
// On the host, with the reference's own functions, point by point: a point that the graph does not know, a point whose mpRefKF the graph
// does not know (GEOM), and the descriptors of the whole list while a keyframe that is not bad has no registered resident frame.
// Returns what ran where (tests, tools).  Throws std::runtime_error when the device call fails.
RefreshStats RefreshMapPoints(const std::vector<ORB_SLAM2::MapPoint *> &vpMapPoints, int what = REFRESH_GEOM | REFRESH_DESC);

} // namespace orbx_adapter

#endif
