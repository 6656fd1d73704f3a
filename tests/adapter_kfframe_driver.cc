// tests/adapter_kfframe_driver.cc -- resident keyframes behind the keyframe-target projection adaptors (orbx_adapter::KeyFrameFrames,
// adapter/ORBmatcher_batch.cc) and the first loop of LocalMapping::SearchInNeighbors as one call (orbx_adapter::FuseBatch,
// adapter/ORBmatcher_fuse.cc), driven on synthetic maps (no image): a handful of keyframes looking at the same world points, the
// keyframes' own map points on some of the features the candidates project to.  Built by tests/test_kf_resident.py against tests/cvstub
// (and, with -DKFFRAME_REPLACE_CHANGES_DESCRIPTOR, tests/cvstub_replace in front of it) and linked with liborbx.so.  Checks, each
// printed as "name value":
//   registered_equal   Fuse, Fuse(Scw), SearchByProjection(Scw) and SearchBySim3 on registered keyframes leave the map state and return the
//                      values of the unregistered (host-pointer) path on a second copy of the scene
//   recycled_rebuilt   keyframes whose content changed at the same address are rebuilt (the creates counter goes up by their number)
//   recycled_equal     ... and the results on them are again those of the unregistered path
//   batch_equal        FuseBatch over 5 targets leaves the state and the counts of the loop `for t: Fuse(target[t], points, th)`
//   batch_launches / batch_researched   FuseBatchStats: one launch; points searched again (0 with the plain stub, >= 1 when Replace
//                      changes the survivor's descriptor)
//   loop_replace_new_by_old / loop_replace_old_by_new / loop_add_observation   what the plain loop did (each must be >= 1)
// Exit status 0 when every check holds.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <stdexcept>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBmatcher.h"
#include "orbx_adapter.h"
#include "orbx_batch.h"

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

static int NT = 5, NP = 360, NF = 460;             // targets, candidate points, features per keyframe (the first NP belong to the points)
static const float FX = 718.856f, FY = 718.856f, CX = 607.1928f, CY = 185.2157f, BF = 386.1448f;

struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> cand, own;      // own[t * NP + i]: keyframe t's own point on feature i (used where the slot rule says so)
    std::vector<MapPoint *> vcand;
};

static cv::Mat vec3(float x, float y, float z)
{
    cv::Mat m(3, 1, CV_32F);
    m.at<float>(0) = x; m.at<float>(1) = y; m.at<float>(2) = z;
    return m;
}

static void set_pose(KeyFrame &kf, int t)
{
    const float a = 0.004f * (float)t, ca = cosf(a), sa = sinf(a);
    kf.Rcw = cv::Mat(3, 3, CV_32F);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) kf.Rcw.at<float>(r, c) = r == c ? 1.f : 0.f;
    kf.Rcw.at<float>(0, 0) = ca; kf.Rcw.at<float>(0, 2) = sa; kf.Rcw.at<float>(2, 0) = -sa; kf.Rcw.at<float>(2, 2) = ca;
    kf.tcw = vec3(0.05f * (float)t, -0.02f * (float)t, 0.1f * (float)t);
    kf.Ow = -kf.Rcw.t() * kf.tcw;
}

static cv::Mat pose44(const KeyFrame &kf)
{
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = r == c ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T.at<float>(r, c) = kf.Rcw.at<float>(r, c);
        T.at<float>(r, 3) = kf.tcw.at<float>(r);
    }
    return T;
}

// (re)fills the world in place: the objects keep their addresses, their content follows from the seed
static void fill_world(World &w, unsigned seed)
{
    g_rng = seed;
    w.kfs.assign(NT, KeyFrame());
    w.cand.assign(NP, MapPoint());
    w.own.assign((size_t)NT * NP, MapPoint());
    w.vcand.assign(NP, static_cast<MapPoint *>(NULL));
    std::vector<float> sf(8, 1.f), s2(8, 1.f), is2(8, 1.f);
    for (int i = 1; i < 8; i++) sf[i] = sf[i - 1] * 1.2f;
    for (int i = 0; i < 8; i++) { s2[i] = sf[i] * sf[i]; is2[i] = 1.f / s2[i]; }
    std::vector<int> oct(NP);
    for (int i = 0; i < NP; i++) {
        MapPoint &P = w.cand[i];
        const float z = urand(8.f, 14.f), u0 = urand(60.f, 1180.f), v0 = urand(40.f, 336.f);
        P.mWorldPos = vec3((u0 - CX) / FX * z, (v0 - CY) / FY * z, z);
        const float dist = (float)cv::norm(P.mWorldPos);
        P.mNormalVector = (1.0 / dist) * P.mWorldPos;
        oct[i] = (int)(rnd() % 8);
        P.mfMaxDistance = dist * powf(1.2f, (float)oct[i] - 0.5f);          // PredictScale = the octave drawn, from every target's distance
        P.mfMinDistance = 0.f;
        P.mDescriptor = cv::Mat(1, 32, CV_8UC1);
        for (int b = 0; b < 32; b++) P.mDescriptor.data[b] = (uint8_t)rnd();
        P.nObs = 2;
        if (i % 23 == 7) P.mbBad = true;                                    // a few candidates are bad from the start
        w.vcand[i] = i % 31 == 11 ? static_cast<MapPoint *>(NULL) : &P;     // and a few slots are empty
    }
    for (int t = 0; t < NT; t++) {
        KeyFrame &kf = w.kfs[t];
        set_pose(kf, t);
        kf.N = NF; kf.fx = FX; kf.fy = FY; kf.cx = CX; kf.cy = CY; kf.mbf = BF;
        kf.mnScaleLevels = 8; kf.mfLogScaleFactor = logf(1.2f);
        kf.mnMinX = 0; kf.mnMinY = 0; kf.mnMaxX = 1241; kf.mnMaxY = 376;
        kf.mvScaleFactors = sf; kf.mvLevelSigma2 = s2; kf.mvInvLevelSigma2 = is2;
        kf.mvKeysUn.assign(NF, cv::KeyPoint());
        kf.mvuRight.assign(NF, -1.f);
        kf.mDescriptors = cv::Mat(NF, 32, CV_8UC1);
        kf.mvpMapPoints.assign(NF, static_cast<MapPoint *>(NULL));
        for (int i = 0; i < NF; i++) {
            cv::KeyPoint &k = kf.mvKeysUn[i];
            k.size = 31.f; k.response = 1.f; k.class_id = -1; k.angle = urand(0.f, 359.f);
            uint8_t *d = kf.mDescriptors.data + 32 * i;
            if (i >= NP) {                                                  // features that belong to no candidate
                k.pt.x = urand(5.f, 1236.f); k.pt.y = urand(5.f, 371.f); k.octave = (int)(rnd() % 8);
                for (int b = 0; b < 32; b++) d[b] = (uint8_t)rnd();
                continue;
            }
            const cv::Mat pc = kf.Rcw * w.cand[i].mWorldPos + kf.tcw;
            const float zc = pc.at<float>(2), u = FX * pc.at<float>(0) / zc + CX, v = FY * pc.at<float>(1) / zc + CY;
            k.pt.x = u + urand(-0.7f, 0.7f); k.pt.y = v + urand(-0.7f, 0.7f);
            k.octave = (oct[i] > 0 && (i + t) % 3 == 0) ? oct[i] - 1 : oct[i];
            if (i % 5 == 0) kf.mvuRight[i] = k.pt.x - BF / zc + urand(-0.3f, 0.3f);
            memcpy(d, w.cand[i].mDescriptor.data, 32);
            for (int f = 0; f < 5; f++) d[rnd() % 31] ^= (uint8_t)(1u << (rnd() % 8));
            const int rule = (i + t) % 4;                                   // 0: the slot is free; 1: an own point with more observations; 2, 3: with fewer
            if (rule == 0) continue;
            MapPoint &O = w.own[(size_t)t * NP + i];
            O.mWorldPos = w.cand[i].mWorldPos.clone(); O.mNormalVector = w.cand[i].mNormalVector.clone();
            O.mfMaxDistance = w.cand[i].mfMaxDistance; O.mfMinDistance = 0.f;
            O.mDescriptor = cv::Mat(1, 32, CV_8UC1);
            memcpy(O.mDescriptor.data, d, 32);
            O.nObs = rule == 1 ? 5 : 1;
            O.mObservations[&kf] = (size_t)i;
            kf.mvpMapPoints[i] = &O;
        }
    }
}

static long id_of(const World &w, const MapPoint *p)
{
    if (!p) return -1;
    if (p >= &w.cand[0] && p < &w.cand[0] + w.cand.size()) return 1000000 + (long)(p - &w.cand[0]);
    if (p >= &w.own[0] && p < &w.own[0] + w.own.size()) return (long)(p - &w.own[0]);
    return -7;
}

static void push_point(const World &w, const MapPoint &p, std::vector<long> &s)
{
    s.push_back(p.mbBad); s.push_back(id_of(w, p.mpReplaced)); s.push_back(p.nObs);
    for (std::map<KeyFrame *, size_t>::const_iterator it = p.mObservations.begin(); it != p.mObservations.end(); ++it) {
        s.push_back((long)(it->first - &w.kfs[0])); s.push_back((long)it->second);
    }
    if (!p.mDescriptor.empty())
        for (int b = 0; b < 32; b++) s.push_back(p.mDescriptor.data[b]);
}

// everything the searches can change, in terms that do not depend on addresses
static std::vector<long> snapshot(const World &w)
{
    std::vector<long> s;
    for (size_t t = 0; t < w.kfs.size(); t++)
        for (size_t i = 0; i < w.kfs[t].mvpMapPoints.size(); i++) s.push_back(id_of(w, w.kfs[t].mvpMapPoints[i]));
    for (size_t i = 0; i < w.cand.size(); i++) push_point(w, w.cand[i], s);
    for (size_t i = 0; i < w.own.size(); i++) push_point(w, w.own[i], s);
    return s;
}

static void push_ids(const World &w, const std::vector<MapPoint *> &v, std::vector<long> &s)
{
    for (size_t i = 0; i < v.size(); i++) s.push_back(id_of(w, v[i]));
}

// the four keyframe-target searches on one world; returns their return values, outputs and the map state
static std::vector<long> four_searches(World &w, std::vector<int> &counts)
{
    std::vector<long> s;
    ORBmatcher m(0.75f, true);
    counts.clear();
    counts.push_back(m.Fuse(&w.kfs[0], w.vcand, 3.f));                                     // LocalMapping::SearchInNeighbors
    std::vector<MapPoint *> good;
    for (size_t i = 0; i < w.vcand.size(); i++) if (w.vcand[i]) good.push_back(w.vcand[i]);
    std::vector<MapPoint *> repl(good.size(), static_cast<MapPoint *>(NULL));
    counts.push_back(m.Fuse(&w.kfs[1], pose44(w.kfs[1]), good, 4.f, repl));                 // LoopClosing::SearchAndFuse
    push_ids(w, repl, s);
    std::vector<MapPoint *> matched(NF, static_cast<MapPoint *>(NULL));
    for (int i = 0; i < NF; i += 7) matched[i] = w.kfs[2].mvpMapPoints[i];
    counts.push_back(m.SearchByProjection(&w.kfs[2], pose44(w.kfs[2]), good, matched, 10));  // LoopClosing::ComputeSim3
    push_ids(w, matched, s);
    std::vector<MapPoint *> m12(NF, static_cast<MapPoint *>(NULL));
    for (int i = 0; i < NF; i += 9) m12[i] = w.kfs[3].mvpMapPoints[i];
    const cv::Mat R12 = w.kfs[3].Rcw * w.kfs[4].Rcw.t();
    const cv::Mat t12 = w.kfs[3].tcw - R12 * w.kfs[4].tcw;
    const float s12 = 1.f;
    counts.push_back(m.SearchBySim3(&w.kfs[3], &w.kfs[4], m12, s12, R12, t12, 7.5f));
    push_ids(w, m12, s);
    for (size_t i = 0; i < counts.size(); i++) s.push_back(counts[i]);
    const std::vector<long> st = snapshot(w);
    s.insert(s.end(), st.begin(), st.end());
    return s;
}

// `bench [reps]`: the first loop of SearchInNeighbors on 20 targets x 1000 points (1200 features per keyframe) three ways, the adaptor's
// own work (projection, staging, surgery) inside the clock, the refill of the map between repetitions outside it; medians per target
static double median_us(std::vector<double> &v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
static int bench(int reps)
{
    NT = 20; NP = 1000; NF = 1200;
    orbx_adapter::KeyFrameFrames &reg = orbx_adapter::KeyFrameFrames::instance();
    World w;
    std::vector<double> t_host, t_res, t_batch;
    std::vector<int> n_host, n_res, n_batch;
    ORBmatcher matcher(0.6f, true);
    for (int r = 0; r < reps + 2; r++) {
        for (int form = 0; form < 3; form++) {
            fill_world(w, 555u);
            std::vector<KeyFrame *> targets;
            for (int t = 0; t < NT; t++) targets.push_back(&w.kfs[t]);
            if (form == 0) reg.clear();
            else for (int t = 0; t < NT; t++) reg.get(targets[t]);       // resident before the clock starts: keyframes are registered once
            std::vector<int> n(NT, 0);
            const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            if (form < 2) for (int t = 0; t < NT; t++) n[t] = matcher.Fuse(targets[t], w.vcand, 3.f);
            else orbx_adapter::FuseBatch(targets, w.vcand, n, 3.f);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / NT;
            if (r >= 2) (form == 0 ? t_host : form == 1 ? t_res : t_batch).push_back(us);
            (form == 0 ? n_host : form == 1 ? n_res : n_batch) = n;
        }
    }
    const bool same = n_host == n_res && n_host == n_batch;
    printf("adaptor_loop_host_pointer_us_per_target %.1f\nadaptor_loop_resident_us_per_target %.1f\nadaptor_fuse_batch_us_per_target %.1f\n",
           median_us(t_host), median_us(t_res), median_us(t_batch));
    printf("adaptor_fused_target0 %d\nadaptor_same_counts %d\n", n_host[0], (int)same);
    reg.clear();
    return same ? 0 : 1;
}

int main(int argc, char **argv)
{
    try {
        if (argc > 1 && strcmp(argv[1], "bench") == 0) return bench(argc > 2 ? atoi(argv[2]) : 30);
        bool ok = true;
        orbx_adapter::KeyFrameFrames &reg = orbx_adapter::KeyFrameFrames::instance();
        {
            World a, b;
            fill_world(a, 4242u);
            fill_world(b, 4242u);
            std::vector<int> ca, cb;
            const std::vector<long> ra = four_searches(a, ca);               // nothing registered: the host-pointer path
            int creates0 = 0, hits0 = 0;
            reg.stats(&creates0, &hits0);
            for (int t = 0; t < NT; t++) reg.get(&b.kfs[t]);
            const std::vector<long> rb = four_searches(b, cb);
            int creates1 = 0, hits1 = 0;
            reg.stats(&creates1, &hits1);
            const bool eq = ra == rb && creates0 == 0 && creates1 == NT && hits1 == 5 && reg.size() == (size_t)NT &&
                            ca[0] > 20 && ca[1] > 20 && ca[2] > 20 && ca[3] > 20;
            printf("counts %d %d %d %d\n", ca[0], ca[1], ca[2], ca[3]);
            printf("registered_equal %d\n", (int)eq);
            // the same addresses, other content (the allocator handed a dead keyframe's address to a new one)
            fill_world(a, 777u);
            fill_world(b, 777u);
            const std::vector<long> ra2 = four_searches(a, ca);
            const std::vector<long> rb2 = four_searches(b, cb);
            int creates2 = 0, hits2 = 0;
            reg.stats(&creates2, &hits2);
            const bool rebuilt = creates2 == creates1 + NT && hits2 == hits1;
            printf("counts_recycled %d %d %d %d\n", ca[0], ca[1], ca[2], ca[3]);
            printf("recycled_rebuilt %d\nrecycled_equal %d\n", (int)rebuilt, (int)(ra2 == rb2 && ra2 != ra && ca[0] > 20));
            ok = ok && eq && rebuilt && ra2 == rb2 && ra2 != ra;
            for (int t = 0; t < NT; t++) reg.drop(&b.kfs[t]);
            ok = ok && reg.size() == 0 && !reg.find(&b.kfs[0]);
        }
        {
            World l, m;
            fill_world(l, 31337u);
            fill_world(m, 31337u);
            std::vector<KeyFrame *> tl, tm;
            for (int t = 0; t < NT; t++) { tl.push_back(&l.kfs[t]); tm.push_back(&m.kfs[t]); }
            ORBmatcher matcher(0.6f, true);
            std::vector<int> nl(NT, 0), nm;
            for (int t = 0; t < NT; t++) nl[t] = matcher.Fuse(tl[t], l.vcand, 3.f);             // src/LocalMapping.cc:549-554
            int launches0 = 0, re0 = 0, launches1 = 0, re1 = 0;
            orbx_adapter::FuseBatchStats(&launches0, &re0);
            orbx_adapter::FuseBatch(tm, m.vcand, nm, 3.f);
            orbx_adapter::FuseBatchStats(&launches1, &re1);
            const bool eq = nl == nm && snapshot(l) == snapshot(m);
            int new_by_old = 0, old_by_new = 0, add_obs = 0;
            for (size_t i = 0; i < l.cand.size(); i++) {
                if (l.cand[i].mbBad && l.cand[i].mpReplaced) new_by_old++;
                add_obs += (int)l.cand[i].mObservations.size();
            }
            for (size_t i = 0; i < l.own.size(); i++) if (l.own[i].mbBad && l.own[i].mpReplaced) old_by_new++;
            printf("fused %d %d %d %d %d\n", nl[0], nl[1], nl[2], nl[3], nl[4]);
            printf("batch_targets %d\nbatch_points %d\n", NT, NP);
            printf("batch_equal %d\nbatch_launches %d\nbatch_researched %d\n", (int)eq, launches1 - launches0, re1 - re0);
            printf("loop_replace_new_by_old %d\nloop_replace_old_by_new %d\nloop_add_observation %d\n", new_by_old, old_by_new, add_obs);
            ok = ok && eq && launches1 - launches0 == 1 && new_by_old >= 1 && old_by_new >= 1 && add_obs >= 1;
#ifdef KFFRAME_REPLACE_CHANGES_DESCRIPTOR
            ok = ok && re1 - re0 >= 1;
#else
            ok = ok && re1 - re0 == 0;
#endif
            reg.clear();
        }
        printf("%s\n", ok ? "adaptor keyframe frames ok" : "adaptor keyframe frames FAILED");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
