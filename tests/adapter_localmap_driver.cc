// tests/adapter_localmap_driver.cc -- Tracking::SearchLocalPoints through the compiled adaptors, two ways on one scene:
//   the reference-shaped route   the second loop of src/Tracking.cc:1433-1463 on the host -- Frame::isInFrustum per point, written with the
//                                structure of src/Frame.cc:310-380 and the float / double steps include/orbx.h fixes for
//                                orbx_mappoints_frustum -- then ORBmatcher(0.8).SearchByProjection(F, vpLocalMapPoints, th), the resident
//                                search adaptor of adapter/ORBmatcher_proj.cc
//   the one-call route           orbx_adapter::SearchLocalPoints (adapter/localmap/LocalMapPoints.cc): resident map points, one ABI call
// Synthetic features (no image).  Built by tests/test_local_points_adapter.py with -DORBX_ADAPTER_CAPTURE against tests/cvstub_localmap in
// front of tests/cvstub, linked with liborbx.so.
//
//   adapter_localmap_driver check
//       both routes on the same scene, then again after a point's descriptor changed, another's position changed, and a third was dropped
//       and a new MapPoint made at its address.  Each round prints "round k equal e ntomatch a b matches a b uploaded u"; equal = F's map,
//       nToMatch, the count, every point's visible counter and captured mTrack* fields identical.  Exit status 0 when every round is equal,
//       matches, and re-sends exactly what changed.
//   adapter_localmap_driver bench NPOINTS NFEATURES REPS
//       adaptor-inclusive timings (std::chrono, medians over REPS, nanoseconds) as "time_a", "time_b", "time_c" lines:
//       a = the reference-shaped route, b = the one call with nothing changed in the table, c = the one call after 5 % of the points
//       changed geometry
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <new>
#include <stdexcept>
#include <vector>

#include "MapPoint.h"
#include "Frame.h"
#include "KeyFrame.h"
#include "ORBmatcher.h"
#include "orbx_adapter.h"
#include "LocalMapPoints.h"

using namespace ORB_SLAM2;

float Frame::fx = 718.856f, Frame::fy = 718.856f, Frame::cx = 607.1928f, Frame::cy = 185.2157f;
float Frame::mnMinX = 0.f, Frame::mnMaxX = 1241.f, Frame::mnMinY = 0.f, Frame::mnMaxY = 376.f;

// MapPoint::PredictScale (reference src/MapPoint.cc): float log, float division, ceil, clamp
namespace ORB_SLAM2 {
static int predict(float maxd, float dist, float logsf, int nlevels)
{
    const float ratio = maxd / dist;
    int n = (int)ceilf(logf(ratio) / logsf);
    if (n < 0) n = 0; else if (n >= nlevels) n = nlevels - 1;
    return n;
}
int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF) { return predict(mfMaxDistance, currentDist, pKF->mfLogScaleFactor, pKF->mnScaleLevels); }
int MapPoint::PredictScale(const float &currentDist, Frame *pF) { return predict(mfMaxDistance, currentDist, pF->mfLogScaleFactor, pF->mnScaleLevels); }
}

// Frame::isInFrustum (src/Frame.cc:310-380), scalar: the reference's cv::Mat expressions restated in the arithmetic include/orbx.h fixes
static bool is_in_frustum(Frame &F, MapPoint *pMP, float viewingCosLimit)
{
    pMP->mbTrackInView = false;
    const cv::Mat P = pMP->GetWorldPos();
    const float X = P.at<float>(0), Y = P.at<float>(1), Z = P.at<float>(2);
    const cv::Mat &R = F.mRcw, &t = F.mtcw, &O = F.mOw;
    const float PcX = ((R.at<float>(0, 0) * X + R.at<float>(0, 1) * Y) + R.at<float>(0, 2) * Z) + t.at<float>(0);
    const float PcY = ((R.at<float>(1, 0) * X + R.at<float>(1, 1) * Y) + R.at<float>(1, 2) * Z) + t.at<float>(1);
    const float PcZ = ((R.at<float>(2, 0) * X + R.at<float>(2, 1) * Y) + R.at<float>(2, 2) * Z) + t.at<float>(2);
    if (PcZ < 0.0f)
        return false;
    const float invz = 1.0f / PcZ;
    const float u = (Frame::fx * PcX) * invz + Frame::cx;
    const float v = (Frame::fy * PcY) * invz + Frame::cy;
    if (u < Frame::mnMinX || u > Frame::mnMaxX)
        return false;
    if (v < Frame::mnMinY || v > Frame::mnMaxY)
        return false;
    if (!std::isfinite(u) || !std::isfinite(v))
        return false;
    const float maxDistance = pMP->GetMaxDistanceInvariance();
    const float minDistance = pMP->GetMinDistanceInvariance();
    const float POx = X - O.at<float>(0), POy = Y - O.at<float>(1), POz = Z - O.at<float>(2);
    const float dist = (float)sqrt(((double)POx * POx + (double)POy * POy) + (double)POz * POz);
    if (dist < minDistance || dist > maxDistance)
        return false;
    const cv::Mat Pn = pMP->GetNormal();
    const float viewCos = (float)((((double)POx * Pn.at<float>(0) + (double)POy * Pn.at<float>(1)) + (double)POz * Pn.at<float>(2)) / (double)dist);
    if (!std::isfinite(viewCos) || viewCos < viewingCosLimit)
        return false;
    const int nPredictedLevel = pMP->PredictScale(dist, &F);
    pMP->mbTrackInView = true;
    pMP->mTrackProjX = u;
    pMP->mTrackProjXR = u - F.mbf * invz;
    pMP->mTrackProjY = v;
    pMP->mnTrackScaleLevel = nPredictedLevel;
    pMP->mTrackViewCos = viewCos;
    return true;
}

// the second loop of Tracking::SearchLocalPoints and its matcher call (src/Tracking.cc:1433-1463)
static int reference_route(Frame &F, const std::vector<MapPoint *> &vp, float th, int &nToMatch)
{
    nToMatch = 0;
    for (size_t i = 0; i < vp.size(); i++) {
        MapPoint *pMP = vp[i];
        if (pMP->mnLastFrameSeen == F.mnId)
            continue;
        if (pMP->isBad())
            continue;
        if (is_in_frustum(F, pMP, 0.5f)) {
            pMP->IncreaseVisible();
            nToMatch++;
        }
    }
    if (nToMatch > 0) {
        ORBmatcher matcher(0.8f);
        return matcher.SearchByProjection(F, vp, th);
    }
    return 0;
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

static void make_frame(Frame &F, int n, unsigned seed)
{
    g_rng = seed;
    F = Frame();
    F.N = n;
    F.mnId = 17;
    F.mvKeys.resize(n);
    F.mDescriptors = cv::Mat(n, 32, CV_8UC1);
    F.mvuRight.assign(n, -1.f);
    for (int i = 0; i < n; i++) {
        cv::KeyPoint &k = F.mvKeys[i];
        k.pt.x = urand(10.f, 1230.f); k.pt.y = urand(10.f, 366.f); k.angle = urand(0.f, 359.f); k.octave = (int)(rnd() % 8);
        k.size = 31.f; k.response = 1.f; k.class_id = -1;
        for (int b = 0; b < 32; b++) F.mDescriptors.data[32 * i + b] = (uint8_t)rnd();
    }
    F.mvKeysUn = F.mvKeys;
    F.mvScaleFactors.assign(8, 1.f);
    for (int i = 1; i < 8; i++) F.mvScaleFactors[i] = F.mvScaleFactors[i - 1] * 1.2f;
    F.mnScaleLevels = 8; F.mfLogScaleFactor = logf(1.2f);
    F.mbf = 386.1448f; F.mb = F.mbf / Frame::fx;
    F.mvpMapPoints.assign(n, static_cast<MapPoint *>(NULL));
    F.mvbOutlier.assign(n, false);
    F.mTcw = pose(0.05f, -0.02f, -0.2f);
    F.UpdatePoseMatrices();
}

// local point i is the back-projection of feature (7 i + 3) mod N, a few bits and a pixel or two away; some are bad, seen already, behind
// the camera, outside their distance range or facing away
static void make_point(MapPoint &P, const Frame &cur, int i)
{
    const int n = cur.N, src = (i * 7 + 3) % n;
    P = MapPoint();
    P.mDescriptor = cv::Mat(1, 32, CV_8UC1);
    memcpy(P.mDescriptor.data, cur.mDescriptors.data + 32 * src, 32);
    for (int k = 0; k < 6; k++) P.mDescriptor.data[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
    P.nObs = i % 4;
    float z = 8.f + (float)(i % 7);
    if (i % 23 == 5) z = -z;                                                  // behind the camera
    const float u = cur.mvKeysUn[src].pt.x + urand(-2.f, 2.f), v = cur.mvKeysUn[src].pt.y + urand(-2.f, 2.f);
    cv::Mat d(3, 1, CV_32F);
    d.at<float>(0) = (u - Frame::cx) / Frame::fx * z - cur.mtcw.at<float>(0); d.at<float>(1) = (v - Frame::cy) / Frame::fy * z - cur.mtcw.at<float>(1);
    d.at<float>(2) = z - cur.mtcw.at<float>(2);
    P.mWorldPos = cur.mRcw.t() * d;
    const cv::Mat PO = P.mWorldPos - cur.mOw;
    const float dist = (float)cv::norm(PO);
    P.mNormalVector = PO / (double)dist;
    if (i % 29 == 7) P.mNormalVector = -P.mNormalVector;                      // faces away
    P.mfMaxDistance = dist * powf(1.2f, (float)cur.mvKeysUn[src].octave - 0.5f);   // PredictScale = the feature's octave
    P.mfMinDistance = P.mfMaxDistance / powf(1.2f, 7.f);
    if (i % 31 == 9) P.mfMaxDistance = dist * 0.5f;                           // beyond 1.2 * mfMaxDistance
    P.mbBad = i % 37 == 11;
    P.mnLastFrameSeen = i % 41 == 13 ? cur.mnId : 0;
}

struct Scene {
    Frame cur;
    std::vector<MapPoint> store;
    std::vector<MapPoint *> vp;
    std::vector<MapPoint *> held;   // F.mvpMapPoints before the search: some features hold observed points (TrackWithMotionModel's)
    std::vector<MapPoint> old;
};

static void make_scene(Scene &s, int npoints, int nfeatures)
{
    make_frame(s.cur, nfeatures, 99u);
    g_rng = 4242u;
    s.store.assign(npoints, MapPoint());
    s.vp.assign(npoints, static_cast<MapPoint *>(NULL));
    for (int i = 0; i < npoints; i++) { make_point(s.store[i], s.cur, i); s.vp[i] = &s.store[i]; }
    s.old.assign(nfeatures, MapPoint());
    s.held.assign(nfeatures, static_cast<MapPoint *>(NULL));
    for (int f = 0; f < nfeatures; f += 11) { s.old[f].nObs = f % 2 ? 2 : 0; s.held[f] = &s.old[f]; }
}

// everything a route leaves behind
struct Outcome {
    std::vector<MapPoint *> map;
    std::vector<int> visible, level;
    std::vector<unsigned char> in_view;
    std::vector<float> track;   // mTrackProjX, Y, XR, mTrackViewCos of the in-view points, compared as bytes
    int ntomatch, nmatches;
    bool operator==(const Outcome &o) const
    {
        return map == o.map && visible == o.visible && level == o.level && in_view == o.in_view && ntomatch == o.ntomatch && nmatches == o.nmatches &&
               track.size() == o.track.size() && (track.empty() || memcmp(&track[0], &o.track[0], 4 * track.size()) == 0);
    }
};

static Outcome run(Scene &s, bool one_call, float th)
{
    Frame &F = s.cur;
    F.mvpMapPoints = s.held;
    for (size_t i = 0; i < s.vp.size(); i++) { s.vp[i]->mnVisible = 1; s.vp[i]->mbTrackInView = false; }
    Outcome o;
    o.nmatches = one_call ? orbx_adapter::SearchLocalPoints(F, s.vp, th, o.ntomatch) : reference_route(F, s.vp, th, o.ntomatch);
    o.map = F.mvpMapPoints;
    for (size_t i = 0; i < s.vp.size(); i++) {
        MapPoint *p = s.vp[i];
        o.visible.push_back(p->mnVisible);
        o.in_view.push_back(p->mbTrackInView ? 1 : 0);
        if (!p->mbTrackInView) continue;
        o.level.push_back(p->mnTrackScaleLevel);
        o.track.push_back(p->mTrackProjX); o.track.push_back(p->mTrackProjY); o.track.push_back(p->mTrackProjXR); o.track.push_back(p->mTrackViewCos);
    }
    return o;
}

static bool round_of(Scene &s, int k, float th, int expect_uploaded)
{
    const Outcome a = run(s, false, th);
    const Outcome b = run(s, true, th);
    const int up = orbx_adapter::LocalMapPoints::instance().last_uploaded();
    printf("round %d equal %d ntomatch %d %d matches %d %d uploaded %d\n", k, (int)(a == b), a.ntomatch, b.ntomatch, a.nmatches, b.nmatches, up);
    return a == b && a.nmatches > 20 && a.ntomatch > a.nmatches && up == expect_uploaded;
}

static int check()
{
    if (!orbx_adapter::kCapture) { fprintf(stderr, "check needs a build with -DORBX_ADAPTER_CAPTURE\n"); return 2; }
    Scene s;
    make_scene(s, 2000, 1000);
    int eligible = 0;
    for (size_t i = 0; i < s.vp.size(); i++) eligible += !s.vp[i]->mbBad && s.vp[i]->mnLastFrameSeen != s.cur.mnId;
    bool ok = round_of(s, 0, 3.f, eligible);             // every eligible point is new to the table
    ok = round_of(s, 1, 5.f, 0) && ok;                   // nothing changed: nothing is re-sent
    // a descriptor changes (ComputeDistinctiveDescriptors), a position changes (bundle adjustment), a point dies and another is allocated at
    // its address -- with and without the SetBadFlag hook having been called
    MapPoint *a = s.vp[100], *b = s.vp[200], *c = s.vp[310], *d = s.vp[400];
    for (int k = 0; k < 32; k++) a->mDescriptor.data[k] ^= 0xFF;
    b->mWorldPos.at<float>(0) += 0.05f;
    orbx_adapter::LocalMapPoints::instance().drop(c);
    c->~MapPoint(); new (c) MapPoint(); make_point(*c, s.cur, 311);
    d->~MapPoint(); new (d) MapPoint(); make_point(*d, s.cur, 402);   // the hook was missed: the shadow notices
    ok = round_of(s, 2, 3.f, 4) && ok;
    ok = round_of(s, 3, 3.f, 0) && ok;
    orbx_adapter::LocalMapPoints::instance().clear();    // Map::clear: every point is new again
    ok = orbx_adapter::LocalMapPoints::instance().size() == 0 && ok;
    ok = round_of(s, 4, 1.f, eligible) && ok;
    printf("%s\n", ok ? "adaptor localmap ok" : "adaptor localmap FAILED");
    return ok ? 0 : 1;
}

static long long median(std::vector<long long> &v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static int bench(int npoints, int nfeatures, int reps)
{
    typedef std::chrono::steady_clock clk;
    Scene s;
    make_scene(s, npoints, nfeatures);
    std::vector<long long> ta, tb, tc;
    int ntm = 0;
    for (int r = -3; r < reps; r++) {            // three warm-up rounds
        Frame &F = s.cur;
        F.mvpMapPoints = s.held;
        clk::time_point t0 = clk::now();
        reference_route(F, s.vp, 3.f, ntm);
        clk::time_point t1 = clk::now();
        F.mvpMapPoints = s.held;
        clk::time_point t2 = clk::now();
        orbx_adapter::SearchLocalPoints(F, s.vp, 3.f, ntm);
        clk::time_point t3 = clk::now();
        for (int i = 0; i < npoints; i += 20) s.vp[(i + (r & 15)) % npoints]->mWorldPos.at<float>(1) += 1e-4f;   // 5 % of the points move
        F.mvpMapPoints = s.held;
        clk::time_point t4 = clk::now();
        orbx_adapter::SearchLocalPoints(F, s.vp, 3.f, ntm);
        clk::time_point t5 = clk::now();
        if (r < 0) continue;
        ta.push_back(std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count());
        tb.push_back(std::chrono::duration_cast<std::chrono::nanoseconds>(t3 - t2).count());
        tc.push_back(std::chrono::duration_cast<std::chrono::nanoseconds>(t5 - t4).count());
    }
    printf("points %d features %d reps %d ntomatch %d uploaded_c %d\n", npoints, nfeatures, reps, ntm, orbx_adapter::LocalMapPoints::instance().last_uploaded());
    printf("time_a %lld\ntime_b %lld\ntime_c %lld\n", median(ta), median(tb), median(tc));
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc >= 2 && !strcmp(argv[1], "check")) return check();
        if (argc == 5 && !strcmp(argv[1], "bench")) return bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        fprintf(stderr, "usage: adapter_localmap_driver check | bench NPOINTS NFEATURES REPS\n");
        return 2;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
