// tests/adapter_sim3opt_driver.cc -- runs the compiled Optimizer::OptimizeSim3 (adapter/sim3opt/OptimizeSim3.cc) on two stand-in keyframes
// read from a text file, and prints what it left: tests/test_sim3opt_adapter.py compares that with the Python call on the same gather.
//   adapter_sim3opt_driver <scene file>
// scene file (floats as hexadecimal bit patterns, doubles as 16 digits): cam1 fx fy cx cy, cam2 likewise, th2, fix_scale (0 / 1), the 8
// doubles of g2oS12 as qx qy qz qw tx ty tz s, R1w (9) t1w (3) R2w (9) t2w (3), N, then per feature i of KF1
//   "kind x1 y1 inv_sigma2_1 x2 y2 inv_sigma2_2 Xw1[3] Xw2[3]"
// kind 1: a pair; 0: vpMatches1[i] NULL; 2: KF1 has no map point at i; 3: KF1's point is bad; 4: the matched point is bad; 5: the matched
// point is not observed in KF2 (i2 < 0).  The matched point of feature i is observed in KF2 at i2 = N - 1 - i, so the i2 lookup matters.
// Output: "ret R", "S12" + 8 doubles as bit patterns, "matches" + N digits (1: vpMatches1[i] non-NULL on return).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <vector>

#include "Optimizer.h"

static float read_bits(FILE *f)
{
    unsigned u = 0;
    if (fscanf(f, "%x", &u) != 1) { fprintf(stderr, "short scene file\n"); exit(3); }
    float v;
    memcpy(&v, &u, 4);
    return v;
}

static double read_bits64(FILE *f)
{
    unsigned long long u = 0;
    if (fscanf(f, "%llx", &u) != 1) { fprintf(stderr, "short scene file\n"); exit(3); }
    double v;
    memcpy(&v, &u, 8);
    return v;
}

static void read_pose(FILE *f, ORB_SLAM2::KeyFrame &kf)
{
    kf.Rcw = cv::Mat(3, 3, CV_32F); kf.tcw = cv::Mat(3, 1, CV_32F);
    for (int k = 0; k < 9; k++) kf.Rcw.at<float>(k / 3, k % 3) = read_bits(f);
    for (int k = 0; k < 3; k++) kf.tcw.at<float>(k) = read_bits(f);
}

static void read_cam(FILE *f, ORB_SLAM2::KeyFrame &kf)
{
    kf.mK = cv::Mat(3, 3, CV_32F);
    for (int k = 0; k < 9; k++) kf.mK.at<float>(k / 3, k % 3) = k == 8 ? 1.f : 0.f;
    kf.mK.at<float>(0, 0) = read_bits(f); kf.mK.at<float>(1, 1) = read_bits(f); kf.mK.at<float>(0, 2) = read_bits(f); kf.mK.at<float>(1, 2) = read_bits(f);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <scene file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 3; }
    using namespace ORB_SLAM2;
    KeyFrame kf1, kf2;
    read_cam(f, kf1); read_cam(f, kf2);
    const float th2 = read_bits(f);
    int fix = 0, N = 0;
    if (fscanf(f, "%d", &fix) != 1) return 3;
    double s[8];
    for (int k = 0; k < 8; k++) s[k] = read_bits64(f);
    g2o::Sim3 S12(Eigen::Quaterniond(s[3], s[0], s[1], s[2]), Eigen::Vector3d(s[4], s[5], s[6]), s[7]);
    read_pose(f, kf1); read_pose(f, kf2);
    if (fscanf(f, "%d", &N) != 1 || N < 0) return 3;
    kf1.N = kf2.N = N;
    kf1.mvKeysUn.resize(N); kf2.mvKeysUn.resize(N);
    kf1.mvInvLevelSigma2.assign(1, 0.f); kf2.mvInvLevelSigma2.assign(1, 0.f);
    kf1.mvpMapPoints.assign(N, NULL); kf2.mvpMapPoints.assign(N, NULL);
    std::vector<MapPoint> points1((size_t)N), points2((size_t)N);
    std::vector<MapPoint *> matches((size_t)N, NULL);
    for (int i = 0; i < N; i++) {
        int kind = 0;
        if (fscanf(f, "%d", &kind) != 1) return 3;
        const int i2 = N - 1 - i;
        // a level per feature: any per-feature value goes through mvInvLevelSigma2[octave]
        kf1.mvKeysUn[i].pt.x = read_bits(f); kf1.mvKeysUn[i].pt.y = read_bits(f);
        kf1.mvKeysUn[i].octave = (int)kf1.mvInvLevelSigma2.size(); kf1.mvInvLevelSigma2.push_back(read_bits(f));
        kf2.mvKeysUn[i2].pt.x = read_bits(f); kf2.mvKeysUn[i2].pt.y = read_bits(f);
        kf2.mvKeysUn[i2].octave = (int)kf2.mvInvLevelSigma2.size(); kf2.mvInvLevelSigma2.push_back(read_bits(f));
        points1[i].mWorldPos = cv::Mat(3, 1, CV_32F); points2[i].mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) points1[i].mWorldPos.at<float>(k) = read_bits(f);
        for (int k = 0; k < 3; k++) points2[i].mWorldPos.at<float>(k) = read_bits(f);
        if (kind != 2) kf1.mvpMapPoints[i] = &points1[i];
        if (kind == 3) points1[i].mbBad = true;
        if (kind == 4) points2[i].mbBad = true;
        if (kind != 5) { points2[i].AddObservation(&kf2, (size_t)i2); kf2.mvpMapPoints[i2] = &points2[i]; }
        if (kind != 0) matches[i] = &points2[i];
    }
    fclose(f);
    int ret;
    try {
        ret = Optimizer::OptimizeSim3(&kf1, &kf2, matches, S12, th2, fix != 0);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    const double out[8] = { S12.rotation().x(), S12.rotation().y(), S12.rotation().z(), S12.rotation().w(),
                            S12.translation()[0], S12.translation()[1], S12.translation()[2], S12.scale() };
    printf("ret %d\nS12", ret);
    for (int k = 0; k < 8; k++) {
        unsigned long long u;
        memcpy(&u, &out[k], 8);
        printf(" %016llx", u);
    }
    printf("\nmatches ");
    for (int i = 0; i < N; i++) putchar(matches[i] ? '1' : '0');
    printf("\nadaptor sim3opt ok\n");
    return 0;
}
