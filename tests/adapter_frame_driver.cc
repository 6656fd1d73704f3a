// tests/adapter_frame_driver.cc -- the resident-frame cache of the per-frame projection adaptors (orbx_adapter::ResidentFrame,
// adapter/ORBmatcher_proj.cc) driven the way Tracking drives it on one Frame: TrackWithMotionModel's SearchByProjection(CurrentFrame,
// LastFrame, th) and, after clearing mvpMapPoints, again at 2*th (src/Tracking.cc:1065,:1072), SearchLocalPoints' SearchByProjection(F,
// vpLocalMapPoints, th) (:1463) and Relocalization's SearchByProjection(CurrentFrame, pKF, sFound, th, ORBdist) (:1763).  Synthetic
// features (no image).  Built by tests/test_frame_resident_gpu.py with -DORBX_ADAPTER_CAPTURE against tests/cvstub and linked with
// liborbx.so.  Checks, each printed as "name value":
//   equal_direct      every search's effect on mvpMapPoints and its count equal a direct host-pointer ABI call on the captured inputs
//   creates / hits    ResidentFrameStats after the four searches (1 / 3)
//   rebuilt           `cur = Frame(other)` at the same address (the next mCurrentFrame) makes the next search build a new resident frame
//   equal_off         SetResidentFrames(false) gives the same results as the resident run
// Exit status 0 when every check holds.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <set>
#include <stdexcept>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBmatcher.h"
#include "orbx_adapter.h"

using namespace ORB_SLAM2;

float Frame::fx = 718.856f, Frame::fy = 718.856f, Frame::cx = 607.1928f, Frame::cy = 185.2157f;
float Frame::mnMinX = 0.f, Frame::mnMaxX = 1241.f, Frame::mnMinY = 0.f, Frame::mnMaxY = 376.f;

// MapPoint::PredictScale (reference src/MapPoint.cc:393-415)
namespace ORB_SLAM2 {
static int predict(float maxd, float dist, float logsf, int nlevels)
{
    int n = (int)ceil(log(maxd / dist) / logsf);
    if (n < 0) n = 0; else if (n >= nlevels) n = nlevels - 1;
    return n;
}
int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF) { return predict(mfMaxDistance, currentDist, pKF->mfLogScaleFactor, pKF->mnScaleLevels); }
int MapPoint::PredictScale(const float &currentDist, Frame *pF) { return predict(mfMaxDistance, currentDist, pF->mfLogScaleFactor, pF->mnScaleLevels); }
}

static unsigned g_rng = 12345u;
static unsigned rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static float urand(float a, float b) { return a + (b - a) * (float)(rnd() & 0xFFFF) / 65535.f; }

static cv::Mat pose(float tx, float ty, float tz)
{
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = r == c ? 1.f : 0.f;
    const float ca = 0.99995f, sa = 0.0099998f;
    T.at<float>(0, 0) = ca; T.at<float>(0, 2) = sa; T.at<float>(2, 0) = -sa; T.at<float>(2, 2) = ca;
    T.at<float>(0, 3) = tx; T.at<float>(1, 3) = ty; T.at<float>(2, 3) = tz;
    return T;
}

static std::vector<float> scale_factors()
{
    std::vector<float> sf(8, 1.f);
    for (int i = 1; i < 8; i++) sf[i] = sf[i - 1] * 1.2f;
    return sf;
}

static void make_frame(Frame &F, int n, unsigned seed)
{
    g_rng = seed;
    F = Frame();
    F.N = n;
    F.mvKeys.resize(n);
    F.mDescriptors = cv::Mat(n, 32, CV_8UC1);
    F.mvuRight.assign(n, -1.f);
    for (int i = 0; i < n; i++) {
        cv::KeyPoint &k = F.mvKeys[i];
        k.pt.x = urand(10.f, 1230.f); k.pt.y = urand(10.f, 366.f); k.angle = urand(0.f, 359.f); k.octave = (int)(rnd() % 8);
        k.size = 31.f; k.response = 1.f; k.class_id = -1;
        for (int b = 0; b < 32; b++) F.mDescriptors.data[32 * i + b] = (uint8_t)rnd();
        if (i % 3 == 0) F.mvuRight[i] = k.pt.x - urand(1.f, 30.f);
    }
    F.mvKeysUn = F.mvKeys;
    F.mvScaleFactors = scale_factors(); F.mnScaleLevels = 8; F.mfLogScaleFactor = log(1.2f);
    F.mbf = 386.1448f; F.mb = F.mbf / Frame::fx;
    F.mvpMapPoints.assign(n, static_cast<MapPoint *>(NULL));
    F.mvbOutlier.assign(n, false);
}

// a copy of `src`'s descriptor with a few bits flipped
static void near_desc(const Frame &src, int i, uint8_t *dst)
{
    memcpy(dst, src.mDescriptors.data + 32 * i, 32);
    for (int k = 0; k < 6; k++) dst[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
}

struct Scene {
    Frame last;
    KeyFrame kf;
    std::vector<MapPoint> store, local, old;
    std::vector<MapPoint *> vlocal;
};

// the last frame's points project near the current frame's features; the local map points sit near them as Frame::isInFrustum left them
static void make_scene(Scene &s, Frame &cur)
{
    const int n = cur.N;
    make_frame(s.last, n, 777u);
    g_rng = 4242u;
    s.store.assign(n, MapPoint());
    s.local.assign(n, MapPoint());
    s.old.assign(n, MapPoint());
    s.vlocal.assign(n, static_cast<MapPoint *>(NULL));
    cur.mTcw = pose(0.05f, -0.02f, -0.2f);
    s.last.mTcw = pose(0.f, 0.f, 0.f);
    const cv::Mat Rcw = cur.mTcw.rowRange(0, 3).colRange(0, 3), tcw = cur.mTcw.rowRange(0, 3).col(3);
    const cv::Mat Ow = -Rcw.t() * tcw;
    for (int i = 0; i < n; i++) {
        const int src = (i * 7 + 3) % n;
        s.last.mvKeys[i].octave = cur.mvKeysUn[src].octave; s.last.mvKeysUn[i] = s.last.mvKeys[i];
        s.last.mvKeysUn[i].angle = fmodf(cur.mvKeysUn[src].angle + urand(-5.f, 5.f) + 360.f, 360.f);
        MapPoint &P = s.store[i];
        P.mDescriptor = cv::Mat(1, 32, CV_8UC1);
        near_desc(cur, src, P.mDescriptor.data);
        P.nObs = i % 4;
        const float z = 8.f + (float)(i % 7), u = cur.mvKeysUn[src].pt.x + urand(-2.f, 2.f), v = cur.mvKeysUn[src].pt.y + urand(-2.f, 2.f);
        cv::Mat d(3, 1, CV_32F);
        d.at<float>(0) = (u - Frame::cx) / Frame::fx * z - tcw.at<float>(0); d.at<float>(1) = (v - Frame::cy) / Frame::fy * z - tcw.at<float>(1);
        d.at<float>(2) = z - tcw.at<float>(2);
        P.mWorldPos = Rcw.t() * d;
        const float dist = (float)cv::norm(P.mWorldPos - Ow);
        P.mfMaxDistance = dist * powf(1.2f, (float)cur.mvKeysUn[src].octave - 0.5f) / 1.2f;   // PredictScale ~ the feature's octave
        P.mfMinDistance = 0.f;
        if (i % 5 != 3) s.last.mvpMapPoints[i] = &P;
        s.last.mvbOutlier[i] = i % 9 == 4;
        MapPoint &L = s.local[i];
        L.mDescriptor = P.mDescriptor.clone();
        L.nObs = i % 3;
        L.mbTrackInView = i % 7 != 3;
        L.mTrackProjX = cur.mvKeysUn[src].pt.x + urand(-1.f, 1.f); L.mTrackProjY = cur.mvKeysUn[src].pt.y + urand(-1.f, 1.f);
        L.mTrackProjXR = cur.mvuRight[src] > 0 ? cur.mvuRight[src] + urand(-1.f, 1.f) : L.mTrackProjX - 7.f;
        L.mnTrackScaleLevel = cur.mvKeysUn[src].octave;
        L.mTrackViewCos = i % 2 ? 0.999f : 0.9f;
        s.vlocal[i] = &L;
        s.old[i].nObs = i % 2 ? 2 : 0;
    }
    s.kf.N = n; s.kf.mvKeysUn = s.last.mvKeysUn; s.kf.mvpMapPoints = s.last.mvpMapPoints;
}

static std::vector<int> held(const std::vector<MapPoint *> &vp, const Scene &s)
{
    std::vector<int> out(vp.size(), -1);
    for (size_t i = 0; i < vp.size(); i++) {
        if (!vp[i]) continue;
        const MapPoint *p = vp[i];
        if (p >= &s.store[0] && p < &s.store[0] + s.store.size()) out[i] = (int)(p - &s.store[0]);
        else if (p >= &s.local[0] && p < &s.local[0] + s.local.size()) out[i] = 100000 + (int)(p - &s.local[0]);
        else out[i] = 200000 + (int)(p - &s.old[0]);
    }
    return out;
}

// the captured inputs of the adaptor's last call, as the host-pointer ABI takes them
struct Captured {
    orbx_frame_feats ff;
    orbx_proj_points pp;
};
static Captured captured()
{
    orbx_adapter::Capture &c = orbx_adapter::capture();
    Captured r;
    memset(&r, 0, sizeof r);
    r.ff.n = (int)c.cx.size();
    if (r.ff.n) {
        r.ff.x = &c.cx[0]; r.ff.y = &c.cy[0]; r.ff.octave = &c.coctave[0]; r.ff.angle = &c.cangle[0]; r.ff.u_right = &c.curight[0];
        r.ff.desc = &c.cdesc[0]; r.ff.occupied = &c.coccupied[0];
    }
    r.ff.min_x = c.bounds[0]; r.ff.min_y = c.bounds[1]; r.ff.max_x = c.bounds[2]; r.ff.max_y = c.bounds[3];
    r.pp.n = (int)c.pu.size();
    if (r.pp.n) {
        r.pp.u = &c.pu[0]; r.pp.v = &c.pv[0]; r.pp.aux = &c.paux[0]; r.pp.level = &c.plevel[0]; r.pp.angle = &c.pangle[0];
        r.pp.view_cos = &c.pview[0]; r.pp.desc = &c.pdesc[0]; r.pp.valid = &c.pvalid[0]; r.pp.has_obs = &c.phas_obs[0];
    }
    return r;
}

// what the adaptor does with a match array (src/ORBmatcher.cc:120, :1500, :1526-1545, :1626, :1672)
static std::vector<MapPoint *> apply(const std::vector<MapPoint *> &before, const std::vector<int32_t> &m, const std::vector<MapPoint *> &points)
{
    std::vector<MapPoint *> out = before;
    for (size_t f = 0; f < out.size(); f++) {
        if (m[f] >= 0) out[f] = points[m[f]];
        else if (m[f] == -2) out[f] = NULL;
    }
    return out;
}

struct Result {
    std::vector<std::vector<int> > held;
    std::vector<int> n;
    bool equal_direct;
};

// the tracking sequence on one Frame; every step is checked against a direct host-pointer ABI call on what the adaptor handed over
static Result track(Frame &cur, Scene &s)
{
    Result r;
    r.equal_direct = true;
    const int dev = orbx_adapter::Device();
    const float th = 7.f;
    std::vector<int32_t> m((size_t)cur.N + 1);
    int nd = 0;
    ORBmatcher matcher(0.9f, true);
    // TrackWithMotionModel: some features hold points already (the motion model's previous pass)
    cur.mvpMapPoints.assign(cur.N, static_cast<MapPoint *>(NULL));
    for (int i = 0; i < cur.N; i += 11) cur.mvpMapPoints[i] = &s.old[i];
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) cur.mvpMapPoints.assign(cur.N, static_cast<MapPoint *>(NULL));   // :1070-1072
        const std::vector<MapPoint *> before = cur.mvpMapPoints;
        const int n = matcher.SearchByProjection(cur, s.last, pass == 0 ? th : 2 * th, false);
        Captured c = captured();
        if (orbx_search_by_projection_last_frame(dev, &c.ff, &c.pp, &cur.mvScaleFactors[0], 8, pass == 0 ? th : 2 * th, 0, cur.mbf, 3, &m[0], &nd) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        r.equal_direct = r.equal_direct && nd == n && apply(before, m, s.last.mvpMapPoints) == cur.mvpMapPoints;
        r.held.push_back(held(cur.mvpMapPoints, s)); r.n.push_back(n);
    }
    // SearchLocalPoints: occupied follows from the motion-model search just made
    {
        ORBmatcher ml(0.8f, true);
        const std::vector<MapPoint *> before = cur.mvpMapPoints;
        const int n = ml.SearchByProjection(cur, s.vlocal, 3.f);
        Captured c = captured();
        if (orbx_search_by_projection_map_points(dev, &c.ff, &c.pp, &cur.mvScaleFactors[0], 8, 3.f, 0.8f, &m[0], &nd) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        r.equal_direct = r.equal_direct && nd == n && apply(before, m, s.vlocal) == cur.mvpMapPoints;
        r.held.push_back(held(cur.mvpMapPoints, s)); r.n.push_back(n);
    }
    // Relocalization's projection search against a keyframe
    {
        const std::vector<MapPoint *> before = cur.mvpMapPoints;
        std::set<MapPoint *> found;
        for (int i = 0; i < cur.N; i++) if (cur.mvpMapPoints[i]) found.insert(cur.mvpMapPoints[i]);
        const int n = matcher.SearchByProjection(cur, &s.kf, found, 10.f, 100);
        Captured c = captured();
        if (orbx_search_by_projection_keyframe(dev, &c.ff, &c.pp, &cur.mvScaleFactors[0], 8, 10.f, 100, 3, &m[0], &nd) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        r.equal_direct = r.equal_direct && nd == n && apply(before, m, s.kf.mvpMapPoints) == cur.mvpMapPoints;
        r.held.push_back(held(cur.mvpMapPoints, s)); r.n.push_back(n);
    }
    return r;
}

int main()
{
    try {
        Frame cur;
        make_frame(cur, 900, 99u);
        Scene s;
        make_scene(s, cur);
        const Result a = track(cur, s);
        int creates = 0, hits = 0;
        orbx_adapter::ResidentFrameStats(&creates, &hits);
        printf("counts %d %d %d %d\n", a.n[0], a.n[1], a.n[2], a.n[3]);
        printf("equal_direct %d\n", (int)a.equal_direct);
        printf("creates %d\nhits %d\n", creates, hits);
        // the next frame replaces the current one in place: same address, other content
        Frame next;
        make_frame(next, 900, 1234u);
        const cv::Mat Tcw = cur.mTcw.clone();
        cur = next;
        cur.mTcw = Tcw;
        Scene s2;
        make_scene(s2, cur);
        const Result b = track(cur, s2);
        int creates2 = 0, hits2 = 0;
        orbx_adapter::ResidentFrameStats(&creates2, &hits2);
        printf("rebuilt %d\n", (int)(creates2 == creates + 1 && hits2 == hits + 3 && b.equal_direct));
        printf("counts_next %d %d %d %d\n", b.n[0], b.n[1], b.n[2], b.n[3]);
        // resident frames off: the host-pointer path gives the same answers
        orbx_adapter::SetResidentFrames(false);
        const Result c = track(cur, s2);
        int creates3 = 0, hits3 = 0;
        orbx_adapter::ResidentFrameStats(&creates3, &hits3);
        printf("equal_off %d\n", (int)(c.held == b.held && c.n == b.n && c.equal_direct && creates3 == creates2 && hits3 == hits2));
        const bool ok = a.equal_direct && creates == 1 && hits == 3 && creates2 == 2 && hits2 == 6 && b.equal_direct && c.held == b.held && c.n == b.n &&
                        a.n[0] > 20 && a.n[1] > 20 && a.n[2] > 20 && a.n[3] > 0;
        printf("%s\n", ok ? "adaptor frame ok" : "adaptor frame FAILED");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
