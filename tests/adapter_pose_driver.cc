// tests/adapter_pose_driver.cc -- runs the compiled Optimizer::PoseOptimization (adapter/pose/PoseOptimization.cc) on a stand-in Frame read
// from a text file, and prints what it left: tests/test_pose_adapter.py compares that with the direct ABI call on the same values.
//   adapter_pose_driver <scene file>
// scene file: "fx fy cx cy mbf", 16 floats of Tcw (as hexadecimal bit patterns), N, then per feature "has x y u_right octave_inv_sigma2 X Y Z"
// (floats as bit patterns; has = 0: mvpMapPoints[i] = NULL).  Output: "ret R", "setpose K", "Tcw" + 16 bit patterns, "outlier" + N digits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <vector>

#include "Optimizer.h"

namespace ORB_SLAM2 {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
std::mutex MapPoint::mGlobalMutex;
}

static float read_bits(FILE *f)
{
    unsigned u = 0;
    if (fscanf(f, "%x", &u) != 1) { fprintf(stderr, "short scene file\n"); exit(3); }
    float v;
    memcpy(&v, &u, 4);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <scene file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 3; }
    using namespace ORB_SLAM2;
    Frame F;
    Frame::fx = read_bits(f); Frame::fy = read_bits(f); Frame::cx = read_bits(f); Frame::cy = read_bits(f); F.mbf = read_bits(f);
    F.mTcw = cv::Mat(4, 4, CV_32F);
    for (int k = 0; k < 16; k++) F.mTcw.at<float>(k / 4, k % 4) = read_bits(f);
    if (fscanf(f, "%d", &F.N) != 1 || F.N < 0) return 3;
    F.mvInvLevelSigma2.assign(1, 0.f);
    std::vector<MapPoint> points((size_t)F.N);
    F.mvKeysUn.resize(F.N); F.mvuRight.resize(F.N); F.mvpMapPoints.assign(F.N, NULL);
    F.mvbOutlier.assign(F.N, true);    // stale flags of the frame before: the function clears those of the correspondences
    for (int i = 0; i < F.N; i++) {
        int has = 0;
        if (fscanf(f, "%d", &has) != 1) return 3;
        F.mvKeysUn[i].pt.x = read_bits(f); F.mvKeysUn[i].pt.y = read_bits(f); F.mvuRight[i] = read_bits(f);
        F.mvKeysUn[i].octave = (int)F.mvInvLevelSigma2.size();
        F.mvInvLevelSigma2.push_back(read_bits(f));      // a level per feature: any per-feature value goes through mvInvLevelSigma2[octave]
        for (int k = 0; k < 3; k++) points[i].mWorldPos.at<float>(k) = read_bits(f);
        if (has) F.mvpMapPoints[i] = &points[i];
    }
    fclose(f);
    int ret;
    try {
        ret = Optimizer::PoseOptimization(&F);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("ret %d\nsetpose %d\nTcw", ret, F.set_pose_calls);
    for (int k = 0; k < 16; k++) {
        unsigned u;
        const float v = F.mTcw.at<float>(k / 4, k % 4);
        memcpy(&u, &v, 4);
        printf(" %08x", u);
    }
    printf("\noutlier ");
    for (int i = 0; i < F.N; i++) putchar(F.mvbOutlier[i] ? '1' : '0');
    printf("\nadaptor pose ok\n");
    return 0;
}
