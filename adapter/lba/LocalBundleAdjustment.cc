// adapter/lba/LocalBundleAdjustment.cc -- void ORB_SLAM2::Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap)
// (reference src/Optimizer.cc:528-862) on the device.  The three lists of :530-582 and their marks are built statement for statement; the
// problem is gathered as :602-734 adds vertices and edges; ONE call of orbx_local_bundle_adjustment replaces g2o between :584 and :825
// (it polls pbStopFlag as optimizer.setForceStopFlag makes g2o do); then vToErase in the reference's order, the erasures and the
// write-back under Map::mMutexMapUpdate (:827-861).  It replaces that one function only: BundleAdjustment and OptimizeEssentialGraph
// have adaptors of their own, adapter/ba/ and adapter/essential/ (INTEGRATION.md).  Its own sub-directory, like adapter/pose/: it needs Optimizer.h and Map.h.
#include "Optimizer.h"

#include <list>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_device.h"

using namespace std;

namespace ORB_SLAM2
{

void Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap)
{
    const long unsigned int id = pKF->mnId;

    // :530-543 the local keyframes: pKF, then its covisible keyframes in their order; every neighbour gets the mark, a bad one no place
    list<KeyFrame*> lLocalKeyFrames(1, pKF);
    pKF->mnBALocalForKF = id;
    const vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (size_t i = 0; i < vNeighKFs.size(); i++) {
        vNeighKFs[i]->mnBALocalForKF = id;
        if (!vNeighKFs[i]->isBad()) lLocalKeyFrames.push_back(vNeighKFs[i]);
    }

    // :545-562 the local points: the matches of the local keyframes, in that order, each good point once
    list<MapPoint*> lLocalMapPoints;
    for (list<KeyFrame*>::iterator k = lLocalKeyFrames.begin(); k != lLocalKeyFrames.end(); ++k) {
        const vector<MapPoint*> vpMPs = (*k)->GetMapPointMatches();
        for (size_t i = 0; i < vpMPs.size(); i++) {
            MapPoint *pMP = vpMPs[i];
            if (!pMP || pMP->isBad() || pMP->mnBALocalForKF == id) continue;
            pMP->mnBALocalForKF = id;
            lLocalMapPoints.push_back(pMP);
        }
    }

    // :564-582 the fixed keyframes: the observers of local points that carry neither mark; a bad one gets the mark and no place
    list<KeyFrame*> lFixedCameras;
    for (list<MapPoint*>::iterator p = lLocalMapPoints.begin(); p != lLocalMapPoints.end(); ++p) {
        const map<KeyFrame*, size_t> observations = (*p)->GetObservations();
        for (map<KeyFrame*, size_t>::const_iterator o = observations.begin(); o != observations.end(); ++o) {
            KeyFrame *pKFi = o->first;
            if (pKFi->mnBALocalForKF == id || pKFi->mnBAFixedForKF == id) continue;
            pKFi->mnBAFixedForKF = id;
            if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
        }
    }

    // the vertices (:602-626): the local keyframes, then the fixed ones; the keyframe with mnId == 0 is fixed wherever it stands
    vector<KeyFrame*> vpKFs;
    map<KeyFrame*,int> kfIndex;
    vector<float> Tcw, cam;
    vector<unsigned char> fixed;
    for (int pass = 0; pass < 2; pass++) {
        list<KeyFrame*> &l = pass == 0 ? lLocalKeyFrames : lFixedCameras;
        for (list<KeyFrame*>::iterator k = l.begin(); k != l.end(); ++k) {
            KeyFrame *pKFi = *k;
            kfIndex[pKFi] = (int)vpKFs.size();
            vpKFs.push_back(pKFi);
            const cv::Mat T = pKFi->GetPose();
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) Tcw.push_back(T.at<float>(r, c));
            const float K[5] = { pKFi->fx, pKFi->fy, pKFi->cx, pKFi->cy, pKFi->mbf };
            cam.insert(cam.end(), K, K + 5);
            fixed.push_back(pass == 1 || pKFi->mnId == 0);
        }
    }

    // the points and their edges (:653-734): one edge per observation in a keyframe that is not bad, in the order of a copy of
    // GetObservations(); vpEdgeKF / vpMapPointEdge of both kinds are one list here, `mono` tells them apart
    vector<MapPoint*> vpPoints(lLocalMapPoints.begin(), lLocalMapPoints.end());
    vector<float> Xw, x, y, ur, isig;
    vector<int> edge_kf, edge_point;
    vector<KeyFrame*> vpEdgeKF;
    vector<MapPoint*> vpMapPointEdge;
    vector<bool> mono;
    for (size_t ip = 0; ip < vpPoints.size(); ip++) {
        MapPoint *pMP = vpPoints[ip];
        const cv::Mat P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) Xw.push_back(P.at<float>(k));
        const map<KeyFrame*, size_t> observations = pMP->GetObservations();
        for (map<KeyFrame*, size_t>::const_iterator o = observations.begin(); o != observations.end(); ++o) {
            KeyFrame *pKFi = o->first;
            if (pKFi->isBad()) continue;                         // :670
            const map<KeyFrame*, int>::const_iterator found = kfIndex.find(pKFi);
            if (found == kfIndex.end())   // g2o would dereference a missing vertex here (a keyframe that stopped being bad since the lists were made)
                throw runtime_error("Optimizer::LocalBundleAdjustment: an observation in a keyframe that is in neither list");
            const cv::KeyPoint &kpUn = pKFi->mvKeysUn[o->second];
            const float kp_ur = pKFi->mvuRight[o->second];
            edge_kf.push_back(found->second); edge_point.push_back((int)ip);
            x.push_back(kpUn.pt.x); y.push_back(kpUn.pt.y); ur.push_back(kp_ur);
            isig.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
            vpEdgeKF.push_back(pKFi); vpMapPointEdge.push_back(pMP);
            mono.push_back(kp_ur < 0);                           // :675
        }
    }

    if (pbStopFlag && *pbStopFlag) return;                       // :736-738

    orbx_lba_problem prob;
    prob.n_kf = (int)vpKFs.size(); prob.Tcw = Tcw.data(); prob.cam = cam.data(); prob.fixed = fixed.data();
    prob.n_points = (int)vpPoints.size(); prob.Xw = Xw.data();
    prob.n_edges = (int)edge_kf.size(); prob.edge_kf = edge_kf.data(); prob.edge_point = edge_point.data();
    prob.x = x.data(); prob.y = y.data(); prob.u_right = ur.data(); prob.inv_sigma2 = isig.data();
    orbx_lba_options opt;
    opt.stop = (const volatile unsigned char *)pbStopFlag;      // a bool is one byte that is 0 or 1
    opt.debug_stop_at_trial = -1;
    vector<float> TcwOut(Tcw.size()), XwOut(Xw.size() + 1);
    vector<unsigned char> flags(edge_kf.size() + 1);
    orbx_lba_report rep;
    if (orbx_local_bundle_adjustment(orbx_adapter::Device(), &prob, &opt, TcwOut.data(), XwOut.data(), flags.data(), NULL, NULL, &rep) != ORBX_OK)
        throw runtime_error(string("Optimizer::LocalBundleAdjustment: ") + orbx_last_error());   // ORBX_E_CAPACITY: more than 256 free keyframes
    if (rep.stopped == 1) return;                                // the flag rose between the test above and the call's own: nothing is written

    // vToErase (:792-825): the monocular edges first, then the stereo ones, each in edge order, without the points that are bad by now
    vector<pair<KeyFrame*, MapPoint*> > vToErase;
    vToErase.reserve(edge_kf.size());
    for (int pass = 0; pass < 2; pass++)
        for (size_t i = 0; i < edge_kf.size(); i++)
            if (mono[i] == (pass == 0) && !vpMapPointEdge[i]->isBad() && (flags[i] & 2))
                vToErase.push_back(make_pair(vpEdgeKF[i], vpMapPointEdge[i]));

    unique_lock<mutex> lock(pMap->mMutexMapUpdate);              // :828
    for (size_t i = 0; i < vToErase.size(); i++) {                // :830-839
        vToErase[i].first->EraseMapPointMatch(vToErase[i].second);
        vToErase[i].second->EraseObservation(vToErase[i].first);
    }
    for (list<KeyFrame*>::iterator k = lLocalKeyFrames.begin(); k != lLocalKeyFrames.end(); ++k) {      // :844-851
        const float *T = &TcwOut[16 * (size_t)kfIndex[*k]];
        cv::Mat pose(4, 4, CV_32F);                              // Converter::toCvMat(SE3quat)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) pose.at<float>(r, c) = T[4 * r + c];
        (*k)->SetPose(pose);
    }
    for (size_t ip = 0; ip < vpPoints.size(); ip++) {            // :854-861
        cv::Mat pos(3, 1, CV_32F);                               // Converter::toCvMat(vPoint->estimate())
        for (int k = 0; k < 3; k++) pos.at<float>(k) = XwOut[3 * ip + k];
        vpPoints[ip]->SetWorldPos(pos);
        vpPoints[ip]->UpdateNormalAndDepth();
    }
}

} // namespace ORB_SLAM2
