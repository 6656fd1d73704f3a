// tests/adapter_lba_driver.cc -- runs the compiled Optimizer::LocalBundleAdjustment (adapter/lba/LocalBundleAdjustment.cc) on a stand-in map
// read from a text file, and prints what it left: tests/test_lba_adapter.py compares that with the direct ABI call on the same values.
//   adapter_lba_driver <scene file>
// scene file (floats as hexadecimal bit patterns): "stop" (the flag's value at the call), "nkf npt", then per keyframe
// "mnId bad fx fy cx cy mbf", 16 floats of Tcw, "nfeat" and per feature "x y u_right inv_sigma2 point" (point -1: no match); then
// "ncovis" and the indices of keyframe 0's covisible keyframes (keyframe 0 is pKF); then per point "bad bad_on_read X Y Z".  A feature
// with a point is an observation of it.  Output: per keyframe "kf i setpose n erase n Tcw" + 16 bit patterns, per point
// "pt j set n update n pos" + 3 bit patterns, "erased k j" per erased (keyframe, point) pair in order.
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

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <scene file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 3; }
    using namespace ORB_SLAM2;
    bool stop = read_int(f) != 0;
    const int nkf = read_int(f), npt = read_int(f);
    std::vector<KeyFrame> kfs((size_t)nkf);      // one array: the pointer order of a std::map<KeyFrame*, ...> is the index order
    std::vector<MapPoint> pts((size_t)npt);
    for (int k = 0; k < nkf; k++) {
        KeyFrame &K = kfs[k];
        K.mnId = (long unsigned int)read_int(f); K.mbBad = read_int(f) != 0;
        K.fx = read_bits(f); K.fy = read_bits(f); K.cx = read_bits(f); K.cy = read_bits(f); K.mbf = read_bits(f);
        K.Tcw = cv::Mat(4, 4, CV_32F);
        for (int q = 0; q < 16; q++) K.Tcw.at<float>(q / 4, q % 4) = read_bits(f);
        const int nfeat = read_int(f);
        K.mvKeysUn.resize(nfeat); K.mvuRight.resize(nfeat); K.mvpMapPoints.assign(nfeat, NULL); K.mvInvLevelSigma2.resize(nfeat);
        for (int i = 0; i < nfeat; i++) {
            K.mvKeysUn[i].pt.x = read_bits(f); K.mvKeysUn[i].pt.y = read_bits(f); K.mvuRight[i] = read_bits(f);
            K.mvKeysUn[i].octave = i;                 // a level per feature: any per-feature value goes through mvInvLevelSigma2[octave]
            K.mvInvLevelSigma2[i] = read_bits(f);
            const int p = read_int(f);
            if (p >= 0) { K.mvpMapPoints[i] = &pts[p]; pts[p].mObservations[&K] = (size_t)i; }
        }
    }
    const int ncovis = read_int(f);
    for (int i = 0; i < ncovis; i++) kfs[0].mvpOrderedConnectedKeyFrames.push_back(&kfs[read_int(f)]);
    for (int j = 0; j < npt; j++) {
        pts[j].mnId = (long unsigned int)j;
        pts[j].mbBad = read_int(f) != 0; pts[j].bad_on_read = read_int(f) != 0;
        for (int q = 0; q < 3; q++) pts[j].mWorldPos.at<float>(q) = read_bits(f);
    }
    fclose(f);
    Map map;
    try {
        Optimizer::LocalBundleAdjustment(&kfs[0], &stop, &map);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    for (int k = 0; k < nkf; k++) {
        printf("kf %d setpose %d erase %d Tcw", k, kfs[k].set_pose_calls, kfs[k].erase_calls);
        for (int q = 0; q < 16; q++) printf(" %08x", bits_of(kfs[k].Tcw.at<float>(q / 4, q % 4)));
        printf("\n");
    }
    for (int j = 0; j < npt; j++) {
        printf("pt %d set %d update %d pos", j, pts[j].set_calls, pts[j].update_calls);
        for (int q = 0; q < 3; q++) printf(" %08x", bits_of(pts[j].mWorldPos.at<float>(q)));
        printf("\n");
    }
    const std::vector<std::pair<KeyFrame *, MapPoint *> > &log = MapPoint::erase_log();
    for (size_t i = 0; i < log.size(); i++) printf("erased %d %d\n", (int)(log[i].first - &kfs[0]), (int)(log[i].second - &pts[0]));
    printf("adaptor lba ok\n");
    return 0;
}
