// adapter/localmap/LocalMapPoints.h -- the local map resident on the device, and Tracking::SearchLocalPoints in one call on it.
//
// Tracking::SearchLocalPoints (reference src/Tracking.cc:1403-1466) calls Frame::isInFrustum on every local map point and then
// ORBmatcher::SearchByProjection(F, vpLocalMapPoints, th).  A map point's position, normal, distance range and descriptor change rarely;
// LocalMapPoints keeps them in an orbx_mappoints table, a slot per MapPoint*, and orbx_adapter::SearchLocalPoints sends a frame's pose,
// one slot and one flag byte per local point, and `occupied` -- the frustum test, the scale prediction and the search run on the device.
//
// Hooks in the reference:
//   MapPoint::SetBadFlag   orbx_adapter::LocalMapPoints::instance().drop(this);
//   Map::clear             orbx_adapter::LocalMapPoints::instance().clear();
//   include/MapPoint.h     void GetFrustumRecord(float *geom8, unsigned char *desc32);   (defined in LocalMapPoints.cc)
// Once the table exists, orbx_adapter::RefreshMapPoints (adapter/mappoint/MapPointRefresh.h) writes refreshed records into it on the device.
#ifndef ORBX_ADAPTER_LOCALMAPPOINTS_H
#define ORBX_ADAPTER_LOCALMAPPOINTS_H

#include <stdint.h>
#include <mutex>
#include <unordered_map>
#include <vector>

#include <orbx.h>

namespace ORB_SLAM2
{
class Frame;
class MapPoint;
}

namespace orbx_adapter
{

class LocalMapPoints
{
public:
    // the process-wide table (ORB-SLAM2 has one Map); its capacity is ORBX_MAPPOINTS_CAPACITY from the environment or 262144 points
    // (16 MiB of table plus 4.25 MiB of upload staging in HBM, and 4.25 MiB of pinned host memory), fixed when the first search creates
    // the table on orbx_adapter::Device()
    static LocalMapPoints &instance();
    explicit LocalMapPoints(int capacity);
    ~LocalMapPoints();

    // MapPoint::SetBadFlag: the point's slot returns to the free list (a no-op for a point that never had one)
    void drop(ORB_SLAM2::MapPoint *pMP);
    // Map::clear: every slot is free again; the device table is kept
    void clear();

    // for orbx_adapter::RefreshMapPoints (adapter/mappoint/MapPointRefresh.h: RefreshTable), which writes the table in place.  lend()
    // takes the lock that SearchLocalPoints holds and returns the table -- or NULL, with nothing held, while there is none; until
    // give_back(), lent_slot() is the slot a point holds (-1: none; nothing is handed out) and lent_refreshed() records that the device
    // now holds these halves of the point's record (what bit 0: geom8, bit 1: desc32), which the point's members equal by then.  No
    // search runs in between, so a search never compares members against a shadow that lags the device.
    orbx_mappoints *lend();
    int lent_slot(ORB_SLAM2::MapPoint *pMP);
    void lent_refreshed(ORB_SLAM2::MapPoint *pMP, int slot, int what, const float *geom8, const unsigned char *desc32);
    void give_back();

    int size();                 // points that hold a slot
    int last_uploaded();        // records the most recent search re-sent (tests, tools)

private:
    friend int SearchLocalPoints(ORB_SLAM2::Frame &F, const std::vector<ORB_SLAM2::MapPoint *> &vpLocalMapPoints, float th, int &nToMatch);
    struct Record { float geom[8]; unsigned char desc[32]; };   // what a slot holds on the device: the host shadow, compared with memcmp
    // the slot of pMP with the device record up to date after flush(): a new point takes a slot, a point whose record differs from the
    // shadow (UpdateNormalAndDepth, bundle adjustment, ComputeDistinctiveDescriptors -- or another MapPoint allocated at a dropped one's
    // address before its drop was seen) is queued for the one orbx_mappoints_set of this search
    int slot_for(ORB_SLAM2::MapPoint *pMP);
    void flush();
    void abandon();
    orbx_mappoints *table();

    std::mutex mu_;
    int capacity_, high_, last_uploaded_;
    orbx_mappoints *table_;
    std::unordered_map<ORB_SLAM2::MapPoint *, int> slot_of_;
    std::vector<int> free_;
    std::vector<Record> shadow_;
    enum { UNKNOWN = 0, SENT = 1, QUEUED = 2 };
    std::vector<unsigned char> known_;        // what the slot's shadow says about the device: nothing, the record it holds, or the record
                                              // this search has queued (it becomes SENT when flush() succeeds, UNKNOWN when it does not)
    std::vector<int32_t> up_slots_;           // the queue of one search
    std::vector<float> up_geom_;
    std::vector<unsigned char> up_desc_;
};

// The second loop of Tracking::SearchLocalPoints and its matcher call (src/Tracking.cc:1433-1463): for every local point that is not
// bad and was not seen by this frame already, Frame::isInFrustum(pMP, 0.5) -> IncreaseVisible() and nToMatch++, then
// ORBmatcher(0.8).SearchByProjection(F, vpLocalMapPoints, th) -- as ONE orbx_frame_search_local_points call on the frame's resident copy.
// F.mvpMapPoints receives the matches; returns the search's count.  Needs resident frames (orbx_adapter::SetResidentFrames).
// The mTrack* fields of the points are NOT written (nothing reads them after this call) unless compiled with -DORBX_ADAPTER_CAPTURE.
int SearchLocalPoints(ORB_SLAM2::Frame &F, const std::vector<ORB_SLAM2::MapPoint *> &vpLocalMapPoints, float th, int &nToMatch);

} // namespace orbx_adapter

#endif
