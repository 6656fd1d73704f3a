// adapter/triangulate/CreateNewMapPoints.cc -- LocalMapping::CreateNewMapPoints' search and triangulation (reference
// src/LocalMapping.cc:302-511) as SearchForTriangulationBatch + ONE triangulation call (adapter/triangulate/CreateNewMapPoints.h).
#include "CreateNewMapPoints.h"

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <string.h>
#include <utility>

#include "KeyFrame.h"
#include "orbx_adapter.h"
#include "orbx_batch.h"
#include "orbx_device.h"

using namespace std;
using ORB_SLAM2::KeyFrame;

namespace orbx_adapter
{

TriKeyFrame::TriKeyFrame(KeyFrame *pKF)
{
    if (!pKF) return;
    const size_t n = (size_t)pKF->N;
    x.resize(n); y.resize(n); octave.resize(n); u_right.resize(n);
    for (size_t i = 0; i < n; i++) {
        const cv::KeyPoint &kp = pKF->mvKeysUn[i];
        x[i] = kp.pt.x; y[i] = kp.pt.y; octave[i] = kp.octave;
        u_right[i] = i < pKF->mvuRight.size() ? pKF->mvuRight[i] : -1.0f;
    }
    if (pKF->mvDepth.size() >= n) depth.assign(pKF->mvDepth.begin(), pKF->mvDepth.begin() + n);
    if (pKF->mvKeys.size() >= n) {            // UnprojectStereo reads mvKeys (src/KeyFrame.cc:659-660)
        raw_x.resize(n); raw_y.resize(n);
        for (size_t i = 0; i < n; i++) { raw_x[i] = pKF->mvKeys[i].pt.x; raw_y[i] = pKF->mvKeys[i].pt.y; }
    }
}

orbx_tri_feats TriKeyFrame::feats() const
{
    orbx_tri_feats f;
    memset(&f, 0, sizeof f);
    f.n = (int)x.size();
    if (f.n) {
        f.x = &x[0]; f.y = &y[0]; f.octave = &octave[0]; f.u_right = &u_right[0];
        f.depth = depth.empty() ? NULL : &depth[0];
        f.raw_x = raw_x.empty() ? NULL : &raw_x[0]; f.raw_y = raw_y.empty() ? NULL : &raw_y[0];
    }
    return f;
}

// :249-263, :311-323: [Rcw | tcw], the camera centre and the intrinsics as the keyframe keeps them
static orbx_tri_view view_of(KeyFrame *pKF)
{
    orbx_tri_view v;
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) v.Tcw[4 * r + c] = R.at<float>(r, c);
        v.Tcw[4 * r + 3] = t.at<float>(r);
        v.Ow[r] = O.at<float>(r);
    }
    v.fx = pKF->fx; v.fy = pKF->fy; v.cx = pKF->cx; v.cy = pKF->cy; v.invfx = pKF->invfx; v.invfy = pKF->invfy; v.mb = pKF->mb; v.mbf = pKF->mbf;
    return v;
}

// mvDepth and mvKeys go to a resident copy once, on its first use here.  KeyFrameFrames rebuilds a copy whose keyframe changed, and a
// new copy can live at an old one's address: an entry counts only while its weak reference still names the frame.
static void attach_depth(const FrameRef &frame, KeyFrame *pKF)
{
    static mutex mu;
    static map<const orbx_frame *, weak_ptr<const orbx_frame> > done;
    unique_lock<mutex> lock(mu);
    map<const orbx_frame *, weak_ptr<const orbx_frame> >::iterator it = done.find(frame.get());
    if (it != done.end() && it->second.lock() == frame) return;
    for (it = done.begin(); it != done.end();)
        if (it->second.expired()) done.erase(it++); else ++it;
    const TriKeyFrame a(pKF);
    const size_t n = a.x.size();
    const vector<float> none(n + 1, -1.0f);  // a keyframe without mvDepth has no stereo feature either: every depth reads "none"
    if (orbx_frame_set_depth(const_cast<orbx_frame *>(frame.get()), a.depth.empty() ? &none[0] : &a.depth[0], a.raw_x.empty() ? NULL : &a.raw_x[0],
                             a.raw_y.empty() ? NULL : &a.raw_y[0]) != ORBX_OK)
        throw std::runtime_error(string("CreateNewMapPointsBatch: ") + orbx_last_error());
    done[frame.get()] = frame;
}

#ifdef ORBX_ADAPTER_CAPTURE
TriCapture &tri_capture()
{
    static TriCapture c;
    return c;
}
#endif

int CreateNewMapPointsBatch(KeyFrame *pKF1, const vector<KeyFrame *> &vpKF2, const vector<cv::Mat> &vF12, vector<NewPoint> &out, float ratioFactor)
{
    out.clear();
    const size_t n2 = vpKF2.size();
    if (n2 == 0) return 0;
    if (pKF1->mvScaleFactors.empty() || pKF1->mvLevelSigma2.size() != pKF1->mvScaleFactors.size())
        throw std::runtime_error("CreateNewMapPointsBatch: the keyframe has no level tables");
    vector<vector<pair<size_t, size_t> > > vvPairs;
    SearchForTriangulationBatch(pKF1, vpKF2, vF12, vvPairs, false, 0.6f, false);   // :247, :309
    size_t cap = 1;
    for (size_t i = 0; i < n2; i++) cap = max(cap, vvPairs[i].size());
    vector<int32_t> pairs(2 * cap * n2, -1);
    vector<int> npairs(n2);
    vector<orbx_tri_view> views(n2);
    for (size_t i = 0; i < n2; i++) {
        npairs[i] = (int)vvPairs[i].size();
        for (size_t k = 0; k < vvPairs[i].size(); k++) {
            pairs[2 * (cap * i + k)] = (int32_t)vvPairs[i][k].first;
            pairs[2 * (cap * i + k) + 1] = (int32_t)vvPairs[i][k].second;
        }
        views[i] = view_of(vpKF2[i]);
    }
    const orbx_tri_view v1 = view_of(pKF1);
    const vector<float> &sf = pKF1->mvScaleFactors, &s2 = pKF1->mvLevelSigma2;   // one extractor's tables for the whole map (src/KeyFrame.cc:37-39)
    vector<uint8_t> status(cap * n2, 0);
    vector<float> x3d(3 * cap * n2, 0.f);
    int n_new = 0;

    // resident when every keyframe of the call is registered
    KeyFrameFrames &reg = KeyFrameFrames::instance();
    vector<FrameRef> frames(1 + n2);
    bool resident = true;
    for (size_t i = 0; resident && i <= n2; i++) {
        frames[i] = reg.find(i ? vpKF2[i - 1] : pKF1);
        resident = (bool)frames[i];
    }
    vector<TriKeyFrame> host;
    if (!resident || kCapture) {
        host.reserve(1 + n2);
        host.push_back(TriKeyFrame(pKF1));
        for (size_t i = 0; i < n2; i++) host.push_back(TriKeyFrame(vpKF2[i]));
    }
    int rc;
    if (resident) {
        vector<const orbx_frame *> f2(n2);
        for (size_t i = 0; i <= n2; i++) {
            attach_depth(frames[i], i ? vpKF2[i - 1] : pKF1);
            if (i) f2[i - 1] = frames[i].get();
        }
        rc = orbx_frame_triangulate(frames[0].get(), &v1, &f2[0], &views[0], (int)n2, &pairs[0], (int)cap, &npairs[0], &sf[0], &s2[0], (int)sf.size(),
                                    ratioFactor, &status[0], &x3d[0], &n_new);
    } else {
        vector<orbx_tri_feats> feats(1 + n2);
        vector<const orbx_tri_feats *> p2(n2);
        for (size_t i = 0; i <= n2; i++) {
            feats[i] = host[i].feats();
            if (i) p2[i - 1] = &feats[i];
        }
        rc = orbx_triangulate_pairs(Device(), &feats[0], &v1, &p2[0], &views[0], (int)n2, &pairs[0], (int)cap, &npairs[0], &sf[0], &s2[0], (int)sf.size(),
                                    ratioFactor, &status[0], &x3d[0], &n_new);
    }
    if (rc != ORBX_OK) throw std::runtime_error(string("CreateNewMapPointsBatch: ") + orbx_last_error());
#ifdef ORBX_ADAPTER_CAPTURE
    {
        TriCapture &c = tri_capture();
        c.resident = resident; c.kfs = host; c.views.assign(1, v1); c.views.insert(c.views.end(), views.begin(), views.end());
        c.pairs = pairs; c.npairs = npairs; c.cap = (int)cap; c.scale_factors = sf; c.level_sigma2 = s2; c.ratio_factor = ratioFactor;
        c.status = status; c.x3d = x3d; c.n_new = n_new;
    }
#endif
    out.reserve((size_t)n_new);
    for (size_t i = 0; i < n2; i++)
        for (size_t k = 0; k < vvPairs[i].size(); k++) {
            if (status[cap * i + k] > 2) continue;               // rejected, or superseded by an earlier neighbour
            NewPoint p;
            p.neighbour = i; p.idx1 = vvPairs[i][k].first; p.idx2 = vvPairs[i][k].second;
            p.x3D = cv::Mat(3, 1, CV_32F);
            for (int r = 0; r < 3; r++) p.x3D.at<float>(r) = x3d[3 * (cap * i + k) + r];
            out.push_back(p);
        }
    return (int)out.size();
}

} // namespace orbx_adapter
