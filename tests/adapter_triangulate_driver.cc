// tests/adapter_triangulate_driver.cc -- orbx_adapter::CreateNewMapPointsBatch (adapter/triangulate/CreateNewMapPoints.cc) on a stub map
// of 1 + 3 keyframes made here: 240 world points seen by all four, descriptors that differ by a few bits per keyframe, monocular and
// stereo features, a tenth of the current keyframe's features holding a map point already.  Built by tests/test_triangulate_adapter.py
// with -DORBX_ADAPTER_CAPTURE against tests/cvstub_triangulate in front of tests/cvstub.
//   adapter_triangulate_driver check
// runs the call with nothing registered (host pointers), repeats the ABI call on the captured inputs and requires `out` to be its created
// pairs in creation order with no idx1 twice; then registers all four keyframes with KeyFrameFrames and requires the resident call to
// give the same `out` bit for bit.  Prints "adaptor triangulate ok".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <stdexcept>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "CreateNewMapPoints.h"
#include "orbx_adapter.h"
#include "orbx_batch.h"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

static const int NP = 240;
static const float FX = 520.9f, FY = 521.0f, CX = 325.1f, CY = 249.7f, MB = 0.08f;

static uint32_t g_lcg = 20240917u;
static uint32_t rnd() { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)rnd() / 16777216.0; }

struct M3 { double m[3][3]; };
static M3 mul(const M3 &a, const M3 &b)
{
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return r;
}
static M3 transpose(const M3 &a)
{
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = a.m[j][i];
    return r;
}
static M3 rot_y(double a)
{
    const M3 r = { { { cos(a), 0, sin(a) }, { 0, 1, 0 }, { -sin(a), 0, cos(a) } } };
    return r;
}

struct Pose { M3 R; double t[3], C[3]; };
static Pose make_pose(const M3 &R, double cx, double cy, double cz)
{
    Pose p;
    p.R = R; p.C[0] = cx; p.C[1] = cy; p.C[2] = cz;
    for (int r = 0; r < 3; r++) p.t[r] = -(R.m[r][0] * cx + R.m[r][1] * cy + R.m[r][2] * cz);
    return p;
}

// LocalMapping::ComputeF12 (src/LocalMapping.cc:712-733): K1^-T [t12]x R12 K2^-1
static cv::Mat compute_f12(const Pose &p1, const Pose &p2)
{
    const M3 R12 = mul(p1.R, transpose(p2.R));
    double t12[3];
    for (int r = 0; r < 3; r++) t12[r] = -(R12.m[r][0] * p2.t[0] + R12.m[r][1] * p2.t[1] + R12.m[r][2] * p2.t[2]) + p1.t[r];
    const M3 tx = { { { 0, -t12[2], t12[1] }, { t12[2], 0, -t12[0] }, { -t12[1], t12[0], 0 } } };
    const M3 Kinv = { { { 1.0 / FX, 0, -CX / FX }, { 0, 1.0 / FY, -CY / FY }, { 0, 0, 1 } } };
    const M3 F = mul(mul(transpose(Kinv), mul(tx, R12)), Kinv);
    cv::Mat f(3, 3, CV_32F);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) f.at<float>(i, j) = (float)F.m[i][j];
    return f;
}

static void fill(KeyFrame &kf, int k, const Pose &p, const std::vector<double> &P, const cv::Mat &desc, std::vector<MapPoint> &store)
{
    kf.N = NP;
    kf.fx = FX; kf.fy = FY; kf.cx = CX; kf.cy = CY; kf.invfx = 1.0f / FX; kf.invfy = 1.0f / FY; kf.mb = MB; kf.mbf = MB * FX;
    kf.mnMinX = -400; kf.mnMinY = -400; kf.mnMaxX = 1040; kf.mnMaxY = 880;
    kf.mfScaleFactor = 1.2f;
    kf.mvScaleFactors.assign(8, 1.0f);
    for (int l = 1; l < 8; l++) kf.mvScaleFactors[l] = kf.mvScaleFactors[l - 1] * 1.2f;
    kf.mvLevelSigma2.resize(8);
    for (int l = 0; l < 8; l++) kf.mvLevelSigma2[l] = kf.mvScaleFactors[l] * kf.mvScaleFactors[l];
    kf.Rcw = cv::Mat(3, 3, CV_32F); kf.tcw = cv::Mat(3, 1, CV_32F); kf.Ow = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) kf.Rcw.at<float>(r, c) = (float)p.R.m[r][c];
        kf.tcw.at<float>(r) = (float)p.t[r]; kf.Ow.at<float>(r) = (float)p.C[r];
    }
    kf.mvKeysUn.resize(NP); kf.mvKeys.resize(NP); kf.mvuRight.assign(NP, -1.0f); kf.mvDepth.assign(NP, -1.0f);
    kf.mDescriptors = cv::Mat(NP, 32, CV_8UC1);
    kf.mvpMapPoints.assign(NP, static_cast<MapPoint *>(NULL));
    store.assign(NP, MapPoint(false));
    for (int q = 0; q < NP; q++) {
        const int i = (q * 7 + k * 31) % NP;     // feature i of keyframe k sees point q
        double pc[3];
        for (int r = 0; r < 3; r++) pc[r] = p.R.m[r][0] * P[3 * q] + p.R.m[r][1] * P[3 * q + 1] + p.R.m[r][2] * P[3 * q + 2] + p.t[r];
        cv::KeyPoint kp;
        kp.pt.x = (float)(FX * pc[0] / pc[2] + CX + uni(-0.3, 0.3));
        kp.pt.y = (float)(FY * pc[1] / pc[2] + CY + uni(-0.3, 0.3));
        kp.size = 31.f; kp.angle = (float)uni(0, 360); kp.response = 1.f; kp.octave = q % 2; kp.class_id = -1;
        kf.mvKeysUn[i] = kp;
        kf.mvKeys[i] = kp;
        kf.mvKeys[i].pt.x += 0.25f;                // an unrectified camera: the raw position is not the undistorted one
        if (q % (k == 0 ? 3 : 4) == 0) {
            kf.mvuRight[i] = kp.pt.x - kf.mbf / (float)pc[2];
            kf.mvDepth[i] = (float)pc[2];
        }
        for (int b = 0; b < 32; b++) {
            uint8_t v = desc.at<uchar>(q, b);
            if (b >= 2 && rnd() % 10 == 0) v ^= (uint8_t)(1u << (rnd() & 7));
            kf.mDescriptors.at<uchar>(i, b) = v;
        }
        kf.mFeatVec.addFeature(100 + (desc.at<uchar>(q, 0) & 15), (unsigned)i);
        if (k == 0 && q % 10 == 0) kf.mvpMapPoints[i] = &store[i];
    }
}

static bool same(const std::vector<orbx_adapter::NewPoint> &a, const std::vector<orbx_adapter::NewPoint> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].neighbour != b[i].neighbour || a[i].idx1 != b[i].idx1 || a[i].idx2 != b[i].idx2) return false;
        for (int r = 0; r < 3; r++)
            if (memcmp(&a[i].x3D.at<float>(r), &b[i].x3D.at<float>(r), 4) != 0) return false;
    }
    return true;
}

static int check()
{
    if (!orbx_adapter::kCapture) { fprintf(stderr, "check needs a build with -DORBX_ADAPTER_CAPTURE\n"); return 2; }
#ifdef ORBX_ADAPTER_CAPTURE
    std::vector<double> P(3 * NP);
    cv::Mat desc(NP, 32, CV_8UC1);
    for (int q = 0; q < NP; q++) {
        const double z = uni(3.0, 8.0);
        P[3 * q] = (uni(80, 560) - CX) / FX * z; P[3 * q + 1] = (uni(80, 400) - CY) / FY * z; P[3 * q + 2] = z;
        for (int b = 0; b < 32; b++) desc.at<uchar>(q, b) = (uint8_t)rnd();
    }
    const Pose poses[4] = { make_pose(rot_y(0.0), 0, 0, 0), make_pose(rot_y(0.02), 0.5, 0.0, 0.0), make_pose(rot_y(0.0), 0.0, -0.4, 0.02),
                            make_pose(rot_y(-0.015), -0.45, 0.1, 0.0) };
    std::vector<KeyFrame> kfs(4);
    std::vector<std::vector<MapPoint> > stores(4);
    for (int k = 0; k < 4; k++) fill(kfs[k], k, poses[k], P, desc, stores[k]);
    std::vector<KeyFrame *> vpN;
    std::vector<cv::Mat> vF12;
    for (int k = 1; k < 4; k++) { vpN.push_back(&kfs[k]); vF12.push_back(compute_f12(poses[0], poses[k])); }
    const float ratioFactor = 1.5f * kfs[0].mfScaleFactor;

    std::vector<orbx_adapter::NewPoint> out_h;
    orbx_adapter::CreateNewMapPointsBatch(&kfs[0], vpN, vF12, out_h, ratioFactor);
    const orbx_adapter::TriCapture c = orbx_adapter::tri_capture();
    if (c.resident || c.kfs.size() != 4 || c.views.size() != 4) { fprintf(stderr, "capture: expected the host-pointer call on 4 keyframes\n"); return 1; }

    // the ABI call on the captured inputs
    std::vector<orbx_tri_feats> feats(4);
    std::vector<const orbx_tri_feats *> p2(3);
    for (int k = 0; k < 4; k++) { feats[k] = c.kfs[k].feats(); if (k) p2[k - 1] = &feats[k]; }
    std::vector<uint8_t> status(c.status.size(), 0);
    std::vector<float> x3d(c.x3d.size(), 0.f);
    int n_new = -1;
    if (orbx_triangulate_pairs(orbx_adapter::Device(), &feats[0], &c.views[0], &p2[0], &c.views[1], 3, &c.pairs[0], c.cap, &c.npairs[0], &c.scale_factors[0],
                               &c.level_sigma2[0], (int)c.scale_factors.size(), c.ratio_factor, &status[0], &x3d[0], &n_new) != ORBX_OK) {
        fprintf(stderr, "orbx_triangulate_pairs: %s\n", orbx_last_error());
        return 1;
    }
    std::vector<orbx_adapter::NewPoint> exp;
    int total = 0, superseded = 0;
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < c.npairs[i]; k++, total++) {
            const size_t at = (size_t)c.cap * i + k;
            superseded += status[at] >= 32;
            if (status[at] > 2) continue;
            orbx_adapter::NewPoint p;
            p.neighbour = (size_t)i; p.idx1 = (size_t)c.pairs[2 * at]; p.idx2 = (size_t)c.pairs[2 * at + 1];
            p.x3D = cv::Mat(3, 1, CV_32F);
            for (int r = 0; r < 3; r++) p.x3D.at<float>(r) = x3d[3 * at + r];
            exp.push_back(p);
        }
    printf("pairs %d created %d superseded %d\n", total, (int)exp.size(), superseded);
    if ((int)exp.size() != n_new || !same(out_h, exp)) { fprintf(stderr, "out differs from the ABI call on the captured inputs\n"); return 1; }
    if (exp.size() < 100 || superseded < 100 || total < 400) { fprintf(stderr, "the scene is too thin: the search found too little\n"); return 1; }
    std::set<size_t> seen;
    for (size_t i = 0; i < out_h.size(); i++) {
        if (!seen.insert(out_h[i].idx1).second) { fprintf(stderr, "feature %zu of the current keyframe gets two points\n", out_h[i].idx1); return 1; }
        if (kfs[0].mvpMapPoints[out_h[i].idx1]) { fprintf(stderr, "feature %zu had a point already\n", out_h[i].idx1); return 1; }
        if (i && out_h[i].neighbour < out_h[i - 1].neighbour) { fprintf(stderr, "not in creation order\n"); return 1; }
    }

    // resident: all four registered
    orbx_adapter::KeyFrameFrames &reg = orbx_adapter::KeyFrameFrames::instance();
    for (int k = 0; k < 4; k++) reg.get(&kfs[k]);
    std::vector<orbx_adapter::NewPoint> out_r, out_r2;
    orbx_adapter::CreateNewMapPointsBatch(&kfs[0], vpN, vF12, out_r, ratioFactor);
    if (!orbx_adapter::tri_capture().resident) { fprintf(stderr, "registered keyframes did not take the resident call\n"); return 1; }
    orbx_adapter::CreateNewMapPointsBatch(&kfs[0], vpN, vF12, out_r2, ratioFactor);   // the depth is attached once
    if (!same(out_r, out_h) || !same(out_r2, out_h)) { fprintf(stderr, "the resident call differs from the host-pointer call\n"); return 1; }
    reg.drop(&kfs[2]);                                                                 // one keyframe not registered: host pointers again
    orbx_adapter::CreateNewMapPointsBatch(&kfs[0], vpN, vF12, out_r, ratioFactor);
    if (orbx_adapter::tri_capture().resident || !same(out_r, out_h)) { fprintf(stderr, "a partly registered map must take the host-pointer call\n"); return 1; }
    reg.clear();
    orbx_adapter::KeyFrameCache::instance().clear();
    printf("adaptor triangulate ok\n");
#endif
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2 || strcmp(argv[1], "check")) { fprintf(stderr, "usage: %s check\n", argv[0]); return 2; }
    try {
        return check();
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
