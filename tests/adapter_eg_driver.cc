// tests/adapter_eg_driver.cc -- runs the compiled Optimizer::OptimizeEssentialGraph (adapter/essential/OptimizeEssentialGraph.cc) on a
// stand-in map read from a text file, and prints what it left: tests/test_eg_adapter.py compares that with the direct ABI call.
//   adapter_eg_driver <scene file>
// scene file (floats as 8, doubles as 16 hexadecimal digits): "bFixScale loop cur nkf npt nconn" (loop, cur: keyframe indices), then per
// keyframe "mnId bad parent" (parent: an index or -1), 16 floats of Tcw, "corrected" + 0 or 1 + 8 doubles, "noncorrected" likewise,
// "nloop" + indices (mspLoopEdges), "ncov" + pairs "index weight" (weights descending); per loop connection "index n" + n indices; per
// point "bad mnCorrectedByKF mnCorrectedReference ref X Y Z" (ref: the reference keyframe's index).
// Output: per keyframe "kf i setpose n unlocked n Tcw" + 16 bit patterns, per point "pt j set n update n pos" + 3 bit patterns.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <vector>

#include "Optimizer.h"

std::mutex *ORB_SLAM2::KeyFrame::watch = NULL;

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

static int read_int(FILE *f)
{
    int v = 0;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short scene file\n"); exit(3); }
    return v;
}

static bool read_sim3(FILE *f, g2o::Sim3 &S)
{
    char word[32];
    if (fscanf(f, "%31s", word) != 1) exit(3);
    if (!read_int(f)) return false;
    double v[8];
    for (int q = 0; q < 8; q++) v[q] = read_bits64(f);
    S = g2o::Sim3(Eigen::Quaterniond(v[3], v[0], v[1], v[2]), Eigen::Vector3d(v[4], v[5], v[6]), v[7]);
    return true;
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
    const bool bFixScale = read_int(f) != 0;
    const int loop = read_int(f), cur = read_int(f), nkf = read_int(f), npt = read_int(f), nconn = read_int(f);
    std::vector<KeyFrame> kfs((size_t)nkf);      // one array: the pointer order of a std::map<KeyFrame*, ...> is the index order
    std::vector<MapPoint> pts((size_t)npt);
    Map map;
    KeyFrame::watch = &map.mMutexMapUpdate;
    LoopClosing::KeyFrameAndPose NonCorrectedSim3, CorrectedSim3;
    std::map<KeyFrame *, std::set<KeyFrame *> > LoopConnections;
    for (int k = 0; k < nkf; k++) {
        KeyFrame &K = kfs[k];
        K.mnId = (long unsigned int)read_int(f); K.mbBad = read_int(f) != 0;
        const int parent = read_int(f);
        if (parent >= 0) { K.mpParent = &kfs[parent]; kfs[parent].mspChildrens.insert(&K); }
        map.mspKeyFrames.push_back(&K);
        K.Tcw = cv::Mat(4, 4, CV_32F);
        for (int q = 0; q < 16; q++) K.Tcw.at<float>(q / 4, q % 4) = read_bits(f);
        g2o::Sim3 S;
        if (read_sim3(f, S)) CorrectedSim3[&K] = S;
        if (read_sim3(f, S)) NonCorrectedSim3[&K] = S;
        const int nloop = read_int(f);
        for (int q = 0; q < nloop; q++) K.mspLoopEdges.insert(&kfs[read_int(f)]);
        const int ncov = read_int(f);
        for (int q = 0; q < ncov; q++) { const int j = read_int(f), w = read_int(f); K.ordered.push_back(std::make_pair(&kfs[j], w)); }
    }
    for (int c = 0; c < nconn; c++) {
        const int k = read_int(f), n = read_int(f);
        for (int q = 0; q < n; q++) LoopConnections[&kfs[k]].insert(&kfs[read_int(f)]);
    }
    for (int j = 0; j < npt; j++) {
        pts[j].mnId = (long unsigned int)j;
        pts[j].mbBad = read_int(f) != 0;
        pts[j].mnCorrectedByKF = (long unsigned int)read_int(f); pts[j].mnCorrectedReference = (long unsigned int)read_int(f);
        pts[j].mpRefKF = &kfs[read_int(f)];
        for (int q = 0; q < 3; q++) pts[j].mWorldPos.at<float>(q) = read_bits(f);
        map.mspMapPoints.push_back(&pts[j]);
    }
    fclose(f);
    try {
        Optimizer::OptimizeEssentialGraph(&map, &kfs[loop], &kfs[cur], NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    if (!map.mMutexMapUpdate.try_lock()) { fprintf(stderr, "mMutexMapUpdate is still held\n"); return 1; }
    map.mMutexMapUpdate.unlock();
    for (int k = 0; k < nkf; k++) {
        printf("kf %d setpose %d unlocked %d Tcw", k, kfs[k].set_pose_calls, kfs[k].unlocked_calls);
        for (int q = 0; q < 16; q++) printf(" %08x", bits_of(kfs[k].Tcw.at<float>(q / 4, q % 4)));
        printf("\n");
    }
    for (int j = 0; j < npt; j++) {
        printf("pt %d set %d update %d pos", j, pts[j].set_calls, pts[j].update_calls);
        for (int q = 0; q < 3; q++) printf(" %08x", bits_of(pts[j].mWorldPos.at<float>(q)));
        printf("\n");
    }
    printf("adaptor eg ok\n");
    return 0;
}
