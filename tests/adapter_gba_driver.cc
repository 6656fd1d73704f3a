// tests/adapter_gba_driver.cc -- runs the compiled Optimizer::GlobalBundleAdjustemnt (adapter/ba/BundleAdjustment.cc) on a stand-in map read
// from a text file, and prints what it left: tests/test_gba_adapter.py compares that with the direct ABI call on the same values.
//   adapter_gba_driver <scene file>
// scene file (floats as hexadecimal bit patterns): "stop nLoopKF nIterations bRobust", "nkf npt", then per keyframe
// "mnId bad in_map fx fy cx cy mbf" (in_map 0: an observer the map's list does not hold), 16 floats of Tcw, "nfeat" and per feature
// "x y u_right inv_sigma2 point" (point -1: no match); then per point "bad bad_on_read X Y Z".  A feature with a point is an observation
// of it.  Output: per keyframe "kf i setpose n mark m Tcw" + 16 bit patterns + "gba" + 16 bit patterns or "-", per point
// "pt j set n update n mark m pos" + 3 bit patterns + "gba" + 3 bit patterns or "-".
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

static int read_int(FILE *f)
{
    int v = 0;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short scene file\n"); exit(3); }
    return v;
}

static unsigned bits_of(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}

static void print_mat(const cv::Mat &m, int n)
{
    if (m.empty()) { printf(" -"); return; }
    for (int q = 0; q < n; q++) printf(" %08x", bits_of(m.at<float>(q / m.cols, q % m.cols)));
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <scene file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 3; }
    using namespace ORB_SLAM2;
    bool stop = read_int(f) != 0;
    const unsigned long nLoopKF = (unsigned long)read_int(f);
    const int nIterations = read_int(f);
    const bool bRobust = read_int(f) != 0;
    const int nkf = read_int(f), npt = read_int(f);
    std::vector<KeyFrame> kfs((size_t)nkf);      // one array: the pointer order of a std::map<KeyFrame*, ...> is the index order
    std::vector<MapPoint> pts((size_t)npt);
    Map map;
    for (int k = 0; k < nkf; k++) {
        KeyFrame &K = kfs[k];
        K.mnId = (long unsigned int)read_int(f); K.mbBad = read_int(f) != 0;
        if (read_int(f)) map.mspKeyFrames.push_back(&K);
        K.fx = read_bits(f); K.fy = read_bits(f); K.cx = read_bits(f); K.cy = read_bits(f); K.mbf = read_bits(f);
        K.Tcw = cv::Mat(4, 4, CV_32F);
        for (int q = 0; q < 16; q++) K.Tcw.at<float>(q / 4, q % 4) = read_bits(f);
        const int nfeat = read_int(f);
        K.mvKeysUn.resize(nfeat); K.mvuRight.resize(nfeat); K.mvInvLevelSigma2.resize(nfeat);
        for (int i = 0; i < nfeat; i++) {
            K.mvKeysUn[i].pt.x = read_bits(f); K.mvKeysUn[i].pt.y = read_bits(f); K.mvuRight[i] = read_bits(f);
            K.mvKeysUn[i].octave = i;                 // a level per feature: any per-feature value goes through mvInvLevelSigma2[octave]
            K.mvInvLevelSigma2[i] = read_bits(f);
            const int p = read_int(f);
            if (p >= 0) pts[p].mObservations[&K] = (size_t)i;
        }
    }
    for (int j = 0; j < npt; j++) {
        pts[j].mnId = (long unsigned int)j;
        pts[j].mbBad = read_int(f) != 0; pts[j].bad_on_read = read_int(f) != 0;
        for (int q = 0; q < 3; q++) pts[j].mWorldPos.at<float>(q) = read_bits(f);
        map.mspMapPoints.push_back(&pts[j]);
    }
    fclose(f);
    try {
        Optimizer::GlobalBundleAdjustemnt(&map, nIterations, &stop, nLoopKF, bRobust);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    for (int k = 0; k < nkf; k++) {
        printf("kf %d setpose %d mark %lu Tcw", k, kfs[k].set_pose_calls, kfs[k].mnBAGlobalForKF);
        print_mat(kfs[k].Tcw, 16);
        printf(" gba");
        print_mat(kfs[k].mTcwGBA, 16);
        printf("\n");
    }
    for (int j = 0; j < npt; j++) {
        printf("pt %d set %d update %d mark %lu pos", j, pts[j].set_calls, pts[j].update_calls, pts[j].mnBAGlobalForKF);
        print_mat(pts[j].mWorldPos, 3);
        printf(" gba");
        print_mat(pts[j].mPosGBA, 3);
        printf("\n");
    }
    printf("adaptor gba ok\n");
    return 0;
}
