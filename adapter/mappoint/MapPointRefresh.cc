// adapter/mappoint/MapPointRefresh.cc -- see MapPointRefresh.h
#include "KeyFrame.h"
#include "MapPoint.h"

#include <string.h>
#include <set>
#include <stdexcept>

#include "MapPointRefresh.h"
#include "MapGraph.h"

using namespace std;

namespace orbx_adapter
{

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

namespace
{
struct Listed { MapPoint *pMP; int point, table_slot, ref; };

// the table of the process, borrowed from its owner: from begin() to end() none of the owner's searches runs
struct Borrowed {
    const RefreshTable *T;
    orbx_mappoints *table;
    Borrowed() : T(NULL), table(NULL) {}
    void borrow(const RefreshTable *t) { T = t; table = t ? t->begin() : NULL; }
    void give_back() { if (table) { table = NULL; T->end(); } }
    ~Borrowed() { give_back(); }
};

// one ABI call over pts[first, last): with the table when `table` is given
void run(orbx_mapgraph *g, orbx_mappoints *table, const vector<Listed> &pts, size_t first, size_t last, orbx_refresh_job job, int what,
         vector<unsigned char> &status, vector<float> &geom, vector<int32_t> &best_kf, vector<int32_t> &best_idx)
{
    const size_t n = last - first;
    if (n == 0) return;
    vector<int32_t> point(n), slot(n), ref(n);
    vector<float> pos(3 * n);
    for (size_t i = 0; i < n; i++) {
        const Listed &l = pts[first + i];
        point[i] = l.point; slot[i] = l.table_slot; ref[i] = l.ref;
        const cv::Mat P = l.pMP->GetWorldPos();
        for (int c = 0; c < 3; c++) pos[3 * i + c] = P.at<float>(c);
    }
    job.what = what; job.n = (int)n; job.point = &point[0]; job.table_slot = table ? &slot[0] : NULL; job.pos = &pos[0]; job.ref_kf = &ref[0];
    if (orbx_mapgraph_refresh_points(g, table, &job, &status[first], &geom[8 * first], &best_kf[first], &best_idx[first], NULL, NULL) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
}
}

RefreshStats RefreshMapPoints(const vector<MapPoint *> &vpMapPoints, int what)
{
    RefreshStats st = { 0, 0, 0, 0 };
    what &= REFRESH_GEOM | REFRESH_DESC;
    if (!what) return st;
    const RefreshFrameOf frame_of = refresh_hooks().frame_of.load();
    MapGraph &G = MapGraph::instance();
    vector<Listed> dev;              // with a table slot first, then without
    vector<MapPoint *> host;
    vector<unsigned char> status;
    vector<float> geom;
    vector<int32_t> best_kf, best_idx;
    vector<KeyFrame *> kf_of;        // by slot, for best_kf
    int dev_what = what;
    size_t with_table = 0;
    // (declared before the graph's lock, so given back behind it: the graph's lock is held only as long as the device call needs it, the
    // table's until the members and the owner's bookkeeping say what the device holds)
    Borrowed lent;
    {
        std::lock_guard<std::mutex> lk(G.mu_);
        G.flush_locked();
        // every keyframe the graph knows, and every slot given up that a row may still name (its keyframe counts as bad, as a keyframe
        // behind SetBadFlag is)
        vector<int32_t> kf_slot;
        vector<float> centre;
        vector<unsigned char> bad;
        vector<std::shared_ptr<const orbx_frame> > keep;
        vector<const orbx_frame *> frame;
        vector<float> sf;
        kf_of.assign((size_t)G.kf_high_, (KeyFrame *)NULL);
        for (int s = 0; s < G.kf_high_; s++) {
            KeyFrame *pKF = (size_t)s < G.kf_of_slot_.size() ? G.kf_of_slot_[s] : NULL;
            if (!pKF) continue;
            unordered_map<KeyFrame *, MapGraph::Id>::iterator it = G.kf_.find(pKF);
            const bool holds = it != G.kf_.end() && it->second.slot == s && it->second.id == pKF->mnId;
            if (!holds && (!G.graph_ || orbx_mapgraph_keyframe_observations(G.graph_, s) <= 0)) continue;
            // (a slot given up whose address another keyframe holds by now -- its object went away without a word -- is listed too, bad
            // and at the origin: the reference would read freed memory there, and a list must not be refused for it)
            const bool gone = !holds && it != G.kf_.end();
            const cv::Mat Ow = gone ? cv::Mat(3, 1, CV_32F) : pKF->GetCameraCenter();
            const bool is_bad = !holds || pKF->isBad();
            std::shared_ptr<const orbx_frame> f;
            if ((what & REFRESH_DESC) && !is_bad) {
                if (frame_of) f = frame_of(pKF);
                if (!f) dev_what &= ~REFRESH_DESC;      // a descriptor the device cannot read: the descriptors of this list stay on the host
            }
            kf_slot.push_back(s); bad.push_back(is_bad ? 1 : 0); keep.push_back(f); frame.push_back(f.get());
            for (int c = 0; c < 3; c++) centre.push_back(Ow.at<float>(c));
            kf_of[s] = gone ? NULL : pKF;
            if (holds && sf.empty()) sf.assign(pKF->mvScaleFactors.begin(), pKF->mvScaleFactors.begin() + pKF->mnScaleLevels);
        }
        // the points
        lent.borrow(refresh_hooks().table.load());
        orbx_mappoints *table = lent.table;
        set<MapPoint *> seen;
        vector<Listed> bare;
        for (size_t i = 0; i < vpMapPoints.size(); i++) {
            MapPoint *pMP = vpMapPoints[i];
            if (!pMP || !seen.insert(pMP).second) continue;
            Listed l = { pMP, G.point_slot(pMP, false), -1, -1 };
            if (l.point >= 0 && (what & REFRESH_GEOM)) {
                KeyFrame *pRef = pMP->GetReferenceKeyFrame();
                l.ref = pRef ? G.kf_slot(pRef) : -1;
            }
            if (l.point < 0 || !dev_what || ((dev_what & REFRESH_GEOM) && l.ref < 0)) { host.push_back(pMP); continue; }
            if (table) l.table_slot = lent.T->slot(pMP);
            (l.table_slot >= 0 ? dev : bare).push_back(l);
        }
        G.flush_locked();            // point_slot and kf_slot may have given up what turned up at a known address
        with_table = dev.size();
        dev.insert(dev.end(), bare.begin(), bare.end());
        const size_t n = dev.size();
        status.assign(n, 0); geom.assign(8 * n, 0.f); best_kf.assign(n, -1); best_idx.assign(n, -1);
        if (n && dev_what) {
            orbx_refresh_job job;
            memset(&job, 0, sizeof job);
            job.nk = (int)kf_slot.size();
            job.kf_slot = kf_slot.empty() ? NULL : &kf_slot[0]; job.kf_centre = centre.empty() ? NULL : &centre[0];
            job.kf_bad = bad.empty() ? NULL : &bad[0]; job.kf_frame = frame.empty() ? NULL : &frame[0];
            job.scale_factors = sf.empty() ? NULL : &sf[0]; job.nlevels = (int)sf.size();
            run(G.graph(), table, dev, 0, with_table, job, dev_what, status, geom, best_kf, best_idx);
            run(G.graph(), NULL, dev, with_table, n, job, dev_what, status, geom, best_kf, best_idx);
            st.abi_calls = (with_table ? 1 : 0) + (n > with_table ? 1 : 0);
        }
    }
    // the members, from what the call handed back: first the points whose record the table holds, then the table goes back
    for (size_t i = 0; i < dev.size(); i++) {
        if (i == with_table) lent.give_back();
        MapPoint *pMP = dev[i].pMP;
        const float *g8 = &geom[8 * i];
        const unsigned char *d32 = NULL;
        if (status[i] & REFRESH_GEOM) {
            cv::Mat normal(3, 1, CV_32F);
            for (int c = 0; c < 3; c++) normal.at<float>(c) = g8[4 + c];
            pMP->SetNormalAndDepth(normal, g8[3], g8[7]);
        }
        if (status[i] & REFRESH_DESC) {
            KeyFrame *pKF = (size_t)best_kf[i] < kf_of.size() ? kf_of[best_kf[i]] : NULL;
            if (!pKF) throw std::runtime_error("orbx_adapter::RefreshMapPoints: the winning descriptor's keyframe has no slot");
            const cv::Mat row = pKF->mDescriptors.row(best_idx[i]);
            pMP->SetDescriptor(row);
            d32 = row.ptr<unsigned char>();
        }
        if (status[i] && i < with_table) lent.T->refreshed(pMP, dev[i].table_slot, status[i], g8, d32);
    }
    lent.give_back();
    if ((what & ~dev_what) & REFRESH_DESC)
        for (size_t i = 0; i < dev.size(); i++) dev[i].pMP->ComputeDistinctiveDescriptors();
    st.on_device = (int)dev.size();
    st.desc_on_host = ((what & ~dev_what) & REFRESH_DESC) ? (int)dev.size() : 0;
    // what the graph does not know: the reference's own functions
    for (size_t i = 0; i < host.size(); i++) {
        if (what & REFRESH_GEOM) host[i]->UpdateNormalAndDepth();
        if (what & REFRESH_DESC) host[i]->ComputeDistinctiveDescriptors();
    }
    st.on_host = (int)host.size();
    return st;
}

} // namespace orbx_adapter
