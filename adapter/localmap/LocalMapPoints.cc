// adapter/localmap/LocalMapPoints.cc -- see LocalMapPoints.h
#include "MapPoint.h"
#include "Frame.h"

#include <stdlib.h>
#include <string.h>
#include <stdexcept>

#include "LocalMapPoints.h"
#include "mappoint/MapPointRefresh.h"
#include "orbx_adapter.h"

using namespace std;

namespace ORB_SLAM2
{

// mWorldPos, mNormalVector and the RAW distances under mMutexPos, mDescriptor under mMutexFeatures: what GetWorldPos / GetNormal /
// Get{Min,Max}DistanceInvariance / GetDescriptor read, without their four cv::Mat clones (and without the 0.8 / 1.2 products, which
// cannot be undone exactly)
void MapPoint::GetFrustumRecord(float *geom8, unsigned char *desc32)
{
    {
        unique_lock<mutex> lock(mMutexPos);
        for (int k = 0; k < 3; k++) {
            geom8[k] = mWorldPos.at<float>(k);
            geom8[4 + k] = mNormalVector.empty() ? 0.f : mNormalVector.at<float>(k);
        }
        geom8[3] = mfMinDistance; geom8[7] = mfMaxDistance;
    }
    unique_lock<mutex> lock(mMutexFeatures);
    if (mDescriptor.empty()) memset(desc32, 0, 32); else memcpy(desc32, mDescriptor.data, 32);
}

} // namespace ORB_SLAM2

namespace orbx_adapter
{

using ORB_SLAM2::Frame;
using ORB_SLAM2::MapPoint;

static orbx_mappoints *refresh_begin() { return LocalMapPoints::instance().lend(); }
static int refresh_slot(MapPoint *pMP) { return LocalMapPoints::instance().lent_slot(pMP); }
static void refresh_refreshed(MapPoint *pMP, int slot, int what, const float *geom8, const unsigned char *desc32)
{
    LocalMapPoints::instance().lent_refreshed(pMP, slot, what, geom8, desc32);
}
static void refresh_end() { LocalMapPoints::instance().give_back(); }
static const RefreshTable g_refresh_table = { &refresh_begin, &refresh_slot, &refresh_refreshed, &refresh_end };

LocalMapPoints &LocalMapPoints::instance()
{
    static LocalMapPoints *m = NULL;     // never destroyed: no HIP call from a static destructor
    static std::once_flag once;
    std::call_once(once, [] {
        const char *env = getenv("ORBX_MAPPOINTS_CAPACITY");
        const int cap = env && *env ? atoi(env) : 0;
        m = new LocalMapPoints(cap > 0 ? cap : 262144);
    });
    return *m;
}

LocalMapPoints::LocalMapPoints(int capacity) : capacity_(capacity), high_(0), last_uploaded_(0), table_(NULL) {}

LocalMapPoints::~LocalMapPoints()
{
    if (table_) orbx_mappoints_destroy(table_);
}

orbx_mappoints *LocalMapPoints::table()
{
    if (!table_) {
        if (orbx_mappoints_create(Device(), capacity_, &table_) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        shadow_.resize((size_t)capacity_);
        known_.assign((size_t)capacity_, (unsigned char)UNKNOWN);
        if (this == &instance()) refresh_hooks().table.store(&g_refresh_table);      // the process's table: RefreshMapPoints writes it in place from now on
    }
    return table_;
}

orbx_mappoints *LocalMapPoints::lend()
{
    mu_.lock();
    if (!table_) mu_.unlock();
    return table_;
}

void LocalMapPoints::give_back() { mu_.unlock(); }

// (the caller holds mu_ through lend())
int LocalMapPoints::lent_slot(MapPoint *pMP)
{
    std::unordered_map<MapPoint *, int>::iterator it = slot_of_.find(pMP);
    return it == slot_of_.end() ? -1 : it->second;
}

void LocalMapPoints::lent_refreshed(MapPoint *pMP, int slot, int what, const float *geom8, const unsigned char *desc32)
{
    std::unordered_map<MapPoint *, int>::iterator it = slot_of_.find(pMP);
    if (it == slot_of_.end() || it->second != slot || known_[slot] != SENT) return;    // nothing known about the slot: the next search sends it whole
    if ((what & REFRESH_GEOM) && geom8) memcpy(shadow_[slot].geom, geom8, sizeof shadow_[slot].geom);
    if ((what & REFRESH_DESC) && desc32) memcpy(shadow_[slot].desc, desc32, sizeof shadow_[slot].desc);
}

void LocalMapPoints::drop(MapPoint *pMP)
{
    std::lock_guard<std::mutex> lk(mu_);
    std::unordered_map<MapPoint *, int>::iterator it = slot_of_.find(pMP);
    if (it == slot_of_.end()) return;
    free_.push_back(it->second);
    slot_of_.erase(it);
}

void LocalMapPoints::clear()
{
    std::lock_guard<std::mutex> lk(mu_);
    slot_of_.clear();
    free_.clear();
    high_ = 0;
    if (!known_.empty()) known_.assign(known_.size(), (unsigned char)UNKNOWN);
}

int LocalMapPoints::size()
{
    std::lock_guard<std::mutex> lk(mu_);
    return (int)slot_of_.size();
}

int LocalMapPoints::last_uploaded()
{
    std::lock_guard<std::mutex> lk(mu_);
    return last_uploaded_;
}

int LocalMapPoints::slot_for(MapPoint *pMP)
{
    int slot;
    std::unordered_map<MapPoint *, int>::iterator it = slot_of_.find(pMP);
    if (it != slot_of_.end()) {
        slot = it->second;
    } else {
        if (!free_.empty()) { slot = free_.back(); free_.pop_back(); }
        else if (high_ < capacity_) slot = high_++;
        else throw std::runtime_error("orbx adaptor: the resident map-point table is full (ORBX_MAPPOINTS_CAPACITY)");
        slot_of_[pMP] = slot;
        known_[slot] = UNKNOWN;
    }
    Record r;
    pMP->GetFrustumRecord(r.geom, r.desc);
    if (known_[slot] == QUEUED || (known_[slot] == SENT && memcmp(&r, &shadow_[slot], sizeof r) == 0))
        return slot;                     // (queued: the point is named twice in one search, its record travels once)
    shadow_[slot] = r;
    known_[slot] = QUEUED;               // the device holds it only once flush() has succeeded
    up_slots_.push_back(slot);
    up_geom_.insert(up_geom_.end(), r.geom, r.geom + 8);
    up_desc_.insert(up_desc_.end(), r.desc, r.desc + 32);
    return slot;
}

void LocalMapPoints::flush()
{
    last_uploaded_ = (int)up_slots_.size();
    if (up_slots_.empty()) return;
    if (orbx_mappoints_set(table_, &up_slots_[0], (int)up_slots_.size(), &up_geom_[0], &up_desc_[0], NULL) != ORBX_OK) {
        abandon();
        throw std::runtime_error(orbx_last_error());
    }
    for (size_t i = 0; i < up_slots_.size(); i++) known_[up_slots_[i]] = SENT;
    up_slots_.clear(); up_geom_.clear(); up_desc_.clear();
}

// the queue did not reach the device (a full table part-way through a search, a failed set): its slots' shadows say nothing about the
// device any more, so the next search sends those points again
void LocalMapPoints::abandon()
{
    for (size_t i = 0; i < up_slots_.size(); i++) known_[up_slots_[i]] = UNKNOWN;
    up_slots_.clear(); up_geom_.clear(); up_desc_.clear();
    last_uploaded_ = 0;
}

typedef char record_is_packed[sizeof(float[8]) + 32 == 64 ? 1 : -1];

int SearchLocalPoints(Frame &F, const vector<MapPoint *> &vpLocalMapPoints, float th, int &nToMatch)
{
    nToMatch = 0;
    orbx_frame *rf = ResidentFrame(F);
    if (!rf)
        throw std::runtime_error("orbx adaptor: SearchLocalPoints needs resident frames (SetResidentFrames(true))");
    LocalMapPoints &M = LocalMapPoints::instance();
    const size_t n = vpLocalMapPoints.size();
    vector<int32_t> slots(n ? n : 1, 0);
    vector<uint8_t> flags(n ? n : 1, 0), in_view(n ? n : 1, 0);
    vector<uint8_t> occ((size_t)(F.N > 0 ? F.N : 1), 0);
    for (int i = 0; i < F.N && i < (int)F.mvpMapPoints.size(); i++) {
        MapPoint *pMP = F.mvpMapPoints[i];
        occ[i] = (pMP && pMP->Observations() > 0) ? 1 : 0;           // src/ORBmatcher.cc:80-82
    }
    float pose[15];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) pose[3 * r + c] = F.mRcw.at<float>(r, c);
        pose[9 + r] = F.mtcw.at<float>(r);
        pose[12 + r] = F.mOw.at<float>(r);
    }
    const float cam[9] = { Frame::fx, Frame::fy, Frame::cx, Frame::cy, F.mbf, Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY };
    vector<int32_t> match((size_t)(F.N > 0 ? F.N : 1));
    int nmatches = 0;
    {
        std::lock_guard<std::mutex> lk(M.mu_);
        orbx_mappoints *table = M.table();
        try {
            for (size_t i = 0; i < n; i++) {
                MapPoint *pMP = vpLocalMapPoints[i];
                if (pMP->mnLastFrameSeen == F.mnId || pMP->isBad())  // src/Tracking.cc:1437-1440
                    continue;
                slots[i] = M.slot_for(pMP);
                flags[i] = (uint8_t)(1 | (pMP->Observations() > 0 ? 2 : 0));
            }
        } catch (...) {
            M.abandon();
            throw;
        }
        M.flush();
        if (orbx_frame_search_local_points(rf, &occ[0], table, &slots[0], &flags[0], (int)n, pose, cam, 0.5f, F.mfLogScaleFactor, &F.mvScaleFactors[0],
                                           (int)F.mvScaleFactors.size(), th, 0.8f, &match[0], &nmatches, &in_view[0]) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
#ifdef ORBX_ADAPTER_CAPTURE
        // the driver's view of what Frame::isInFrustum would have left in the points
        vector<float> u(n ? n : 1), v(n ? n : 1), xr(n ? n : 1), vc(n ? n : 1);
        vector<int32_t> lvl(n ? n : 1);
        vector<uint8_t> elig(n ? n : 1), iv2(n ? n : 1);
        for (size_t i = 0; i < n; i++) elig[i] = flags[i] & 1;
        if (orbx_mappoints_frustum(table, &slots[0], &elig[0], (int)n, pose, cam, 0.5f, F.mfLogScaleFactor, (int)F.mvScaleFactors.size(), &iv2[0], &u[0], &v[0],
                                   &xr[0], &lvl[0], &vc[0]) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        for (size_t i = 0; i < n; i++) {
            if (!elig[i]) continue;
            MapPoint *pMP = vpLocalMapPoints[i];
            pMP->mbTrackInView = iv2[i] != 0;
            if (!iv2[i]) continue;
            pMP->mTrackProjX = u[i]; pMP->mTrackProjY = v[i]; pMP->mTrackProjXR = xr[i]; pMP->mnTrackScaleLevel = lvl[i]; pMP->mTrackViewCos = vc[i];
        }
#endif
    }
    for (size_t i = 0; i < n; i++)
        if (in_view[i]) {
            vpLocalMapPoints[i]->IncreaseVisible();                  // :1445-1448
            nToMatch++;
        }
    for (int f = 0; f < F.N; f++)
        if (match[f] >= 0)
            F.mvpMapPoints[f] = vpLocalMapPoints[match[f]];          // src/ORBmatcher.cc:120
    return nmatches;
}

} // namespace orbx_adapter
