// adapter/ba/BundleAdjustment.cc -- ORB_SLAM2::Optimizer::GlobalBundleAdjustemnt and ORB_SLAM2::Optimizer::BundleAdjustment (reference
// src/Optimizer.cc:48-281) on the device.  The problem is gathered as :85-224 adds vertices and edges; ONE call of orbx_bundle_adjustment
// replaces g2o between :67 and :232 (it polls pbStopFlag as optimizer.setForceStopFlag makes g2o do); then the recovery loops of :236-279.
// It replaces these two functions only: OptimizeEssentialGraph has its own adaptor, adapter/essential/ (INTEGRATION.md).  Its own sub-directory, like
// adapter/lba/: it needs Optimizer.h and Map.h.
// Stated deviation: an observation in a good keyframe that is not in vpKFs but has mnId <= maxKFid makes the reference attach the edge to a
// vertex that does not exist (optimizer.vertex() returns NULL); here that observation is skipped.
#include "Optimizer.h"

#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_device.h"

using namespace std;

namespace ORB_SLAM2
{

void Optimizer::GlobalBundleAdjustemnt(Map *pMap, int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust)
{
    vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
    vector<MapPoint*> vpMP = pMap->GetAllMapPoints();
    BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}

void Optimizer::BundleAdjustment(const vector<KeyFrame*> &vpKFs, const vector<MapPoint*> &vpMP, int nIterations, bool *pbStopFlag,
                                 const unsigned long nLoopKF, const bool bRobust)
{
    // the keyframe vertices (:85-99): vpKFs in order without the bad ones; the keyframe with mnId == 0 is fixed wherever it stands
    map<KeyFrame*,int> kfIndex;
    vector<float> Tcw, cam;
    vector<unsigned char> fixed;
    long unsigned int maxKFid = 0;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        kfIndex[pKF] = (int)fixed.size();
        const cv::Mat T = pKF->GetPose();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) Tcw.push_back(T.at<float>(r, c));
        const float K[5] = { pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf };
        cam.insert(cam.end(), K, K + 5);
        fixed.push_back(pKF->mnId == 0);
        if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
    }

    // the point vertices and their edges (:106-224): vpMP in order without the bad ones, one edge per observation in a keyframe that is
    // not bad and not newer than maxKFid, in the order of a copy of GetObservations()
    vector<int> pointIndex(vpMP.size(), -1);
    vector<float> Xw, x, y, ur, isig;
    vector<int> edge_kf, edge_point;
    int nPoints = 0;
    for (size_t i = 0; i < vpMP.size(); i++) {
        MapPoint *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        const cv::Mat P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) Xw.push_back(P.at<float>(k));
        pointIndex[i] = nPoints;
        const map<KeyFrame*, size_t> observations = pMP->GetObservations();
        for (map<KeyFrame*, size_t>::const_iterator o = observations.begin(); o != observations.end(); ++o) {
            KeyFrame *pKF = o->first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;   // :131
            const map<KeyFrame*, int>::const_iterator found = kfIndex.find(pKF);
            if (found == kfIndex.end()) continue;                // the stated deviation
            const cv::KeyPoint &kpUn = pKF->mvKeysUn[o->second];
            edge_kf.push_back(found->second); edge_point.push_back(nPoints);
            x.push_back(kpUn.pt.x); y.push_back(kpUn.pt.y); ur.push_back(pKF->mvuRight[o->second]);
            isig.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
        }
        nPoints++;
    }

    vector<float> TcwOut(Tcw.size()), XwOut(Xw.size() + 1);
    vector<unsigned char> included((size_t)nPoints + 1);
    if (!fixed.empty()) {                                        // an optimiser without a vertex does nothing (optimize returns at once)
        orbx_lba_problem prob;
        prob.n_kf = (int)fixed.size(); prob.Tcw = Tcw.data(); prob.cam = cam.data(); prob.fixed = fixed.data();
        prob.n_points = nPoints; prob.Xw = Xw.data();
        prob.n_edges = (int)edge_kf.size(); prob.edge_kf = edge_kf.data(); prob.edge_point = edge_point.data();
        prob.x = x.data(); prob.y = y.data(); prob.u_right = ur.data(); prob.inv_sigma2 = isig.data();
        orbx_ba_options opt;
        opt.stop = (const volatile unsigned char *)pbStopFlag;  // a bool is one byte that is 0 or 1
        opt.debug_stop_at_trial = -1;
        opt.iterations = nIterations;
        opt.robust = bRobust;
        if (orbx_bundle_adjustment(orbx_adapter::Device(), &prob, &opt, TcwOut.data(), XwOut.data(), included.data(), NULL, NULL, NULL) != ORBX_OK)
            throw runtime_error(string("Optimizer::BundleAdjustment: ") + orbx_last_error());   // ORBX_E_CAPACITY: a map beyond the limits
    }

    for (size_t i = 0; i < vpKFs.size(); i++) {                   // :236-253
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const map<KeyFrame*, int>::const_iterator found = kfIndex.find(pKF);
        if (found == kfIndex.end()) continue;                    // bad when the vertices were made: the reference would read a NULL vertex
        const float *T = &TcwOut[16 * (size_t)found->second];
        cv::Mat pose(4, 4, CV_32F);                              // Converter::toCvMat(SE3quat)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) pose.at<float>(r, c) = T[4 * r + c];
        if (nLoopKF == 0) pKF->SetPose(pose);
        else {
            pKF->mTcwGBA.create(4, 4, CV_32F);
            pose.copyTo(pKF->mTcwGBA);
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (size_t i = 0; i < vpMP.size(); i++) {                    // :257-279
        const int ip = pointIndex[i];
        if (ip < 0 || !included[ip]) continue;                   // vbNotIncludedMP; a point that was bad at :109 has no vertex either
        MapPoint *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        cv::Mat pos(3, 1, CV_32F);                               // Converter::toCvMat(vPoint->estimate())
        for (int k = 0; k < 3; k++) pos.at<float>(k) = XwOut[3 * (size_t)ip + k];
        if (nLoopKF == 0) {
            pMP->SetWorldPos(pos);
            pMP->UpdateNormalAndDepth();
        } else {
            pMP->mPosGBA.create(3, 1, CV_32F);
            pos.copyTo(pMP->mPosGBA);
            pMP->mnBAGlobalForKF = nLoopKF;
        }
    }
}

} // namespace ORB_SLAM2
