// adapter/essential/OptimizeEssentialGraph.cc -- ORB_SLAM2::Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:885-1153) on the
// device.  Vertices and edges are gathered as :914-1092 add them; ONE call of orbx_optimize_essential_graph2 replaces g2o between :891 and
// :1096 and does the arithmetic of the two recovery loops; then, under mMutexMapUpdate, SetPose, SetWorldPos and UpdateNormalAndDepth as
// :1098-1152.  Graph selection stays here because it walks KeyFrame pointers: GetWeight < minFeat, parents, GetLoopEdges,
// GetCovisiblesByWeight, sInsertedEdges.  Its own sub-directory, like adapter/ba/: it needs Optimizer.h, Map.h and LoopClosing.h.
// Stated deviations:
//  - The reference's normal-edge loop (:992-1092) does not test isBad(), and its loop-connection loop (:958-989) does not either: an edge
//    that touches a bad keyframe would be attached to a vertex that does not exist (optimizer.vertex() returns NULL).  Here a bad keyframe
//    has no vertex and an edge touching one is skipped; the recovery loop (:1101), which would read that NULL vertex, passes it over.
//  - A map point whose reference keyframe (nIDr) has no vertex is left as it is; the reference would correct it with two
//    default-constructed Sim3s.
//  - The points' positions are read before the call, not under the lock behind it (LocalMapping stands still during CorrectLoop); a point
//    that has turned bad by then is passed over, as :1126 does.
// -DORBX_EG_ORDER_BY_ID: the keyframes are indexed in mnId order (g2o's own vertex ids are the mnIds), not in the order of
// Map::GetAllKeyFrames, which is the pointer order of a std::set<KeyFrame*>.  The call's solver (ORBX_EG_SOLVER_AUTO) stores the system as
// an envelope in keyframe order; that envelope is narrow in creation order only, and orbx_eg_envelope tells what an order costs.
#include "Optimizer.h"

#include <algorithm>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_device.h"

using namespace std;

namespace ORB_SLAM2
{

#ifdef ORBX_EG_ORDER_BY_ID
static bool LessById(const KeyFrame *a, const KeyFrame *b) { return a->mnId < b->mnId; }
#endif

static void PushSim3(vector<double> &v, const g2o::Sim3 &S)
{
    v.push_back(S.rotation().x()); v.push_back(S.rotation().y()); v.push_back(S.rotation().z()); v.push_back(S.rotation().w());
    v.push_back(S.translation()[0]); v.push_back(S.translation()[1]); v.push_back(S.translation()[2]);
    v.push_back(S.scale());
}

void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                       const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const map<KeyFrame *, set<KeyFrame *> > &LoopConnections, const bool &bFixScale)
{
#ifdef ORBX_EG_ORDER_BY_ID
    vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
    sort(vpKFs.begin(), vpKFs.end(), LessById);
#else
    const vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
#endif
    const vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
    const int minFeat = 100;

    // the keyframe vertices (:914-950): vpKFs in order without the bad ones
    map<KeyFrame*,int> kfIndex;
    map<long unsigned int,int> idIndex;                          // nIDr is an mnId (:1129-1138)
    vector<float> Tcw;
    vector<unsigned char> fixed;
    vector<int> corrected, noncorrected;
    vector<double> Sc, Sn;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int k = (int)fixed.size();
        kfIndex[pKF] = k; idIndex[pKF->mnId] = k;
        const cv::Mat T = pKF->GetPose();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) Tcw.push_back(T.at<float>(r, c));
        fixed.push_back(pKF == pLoopKF);
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) { corrected.push_back((int)(Sc.size() / 8)); PushSim3(Sc, it->second); }
        else corrected.push_back(-1);
        it = NonCorrectedSim3.find(pKF);
        if (it != NonCorrectedSim3.end()) { noncorrected.push_back((int)(Sn.size() / 8)); PushSim3(Sn, it->second); }
        else noncorrected.push_back(-1);
    }

    vector<int> edge_i, edge_j;
    vector<unsigned char> edge_kind;
    struct AddEdge {
        const map<KeyFrame*,int> &index; vector<int> &ei, &ej; vector<unsigned char> &kind;
        void operator()(KeyFrame *v0, KeyFrame *v1, int k) const
        {
            const map<KeyFrame*,int>::const_iterator a = index.find(v0), b = index.find(v1);
            if (a == index.end() || b == index.end()) return;    // the stated deviation
            ei.push_back(a->second); ej.push_back(b->second); kind.push_back((unsigned char)k);
        }
    } addEdge = { kfIndex, edge_i, edge_j, edge_kind };

    // the loop-connection edges (:958-989)
    set<pair<long unsigned int,long unsigned int> > sInsertedEdges;
    for (map<KeyFrame *, set<KeyFrame *> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const set<KeyFrame*> &spConnections = mit->second;
        for (set<KeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            addEdge(pKF, *sit, 0);
            sInsertedEdges.insert(make_pair(min(nIDi, nIDj), max(nIDi, nIDj)));
        }
    }

    // the normal edges (:992-1092)
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame *pKF = vpKFs[i];
        if (!kfIndex.count(pKF)) continue;                       // the stated deviation
        KeyFrame *pParentKF = pKF->GetParent();
        if (pParentKF) addEdge(pKF, pParentKF, 1);               // spanning tree
        const set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();
        for (set<KeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++)
            if ((*sit)->mnId < pKF->mnId) addEdge(pKF, *sit, 1);
        const vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (vector<KeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame *pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(make_pair(min(pKF->mnId, pKFn->mnId), max(pKF->mnId, pKFn->mnId)))) continue;
                    addEdge(pKF, pKFn, 1);
                }
            }
        }
    }

    // the map points and their reference keyframes (:1122-1138)
    vector<int> pointIndex(vpMPs.size(), -1), point_ref;
    vector<float> Xw;
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        long unsigned int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        const map<long unsigned int,int>::const_iterator found = idIndex.find(nIDr);
        if (found == idIndex.end()) continue;                    // the stated deviation
        const cv::Mat P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) Xw.push_back(P.at<float>(k));
        pointIndex[i] = (int)point_ref.size();
        point_ref.push_back(found->second);
    }

    if (fixed.empty()) return;
    vector<float> TcwOut(Tcw.size()), XwOut(Xw.size() + 1);
    orbx_eg_problem prob;
    prob.n_kf = (int)fixed.size(); prob.Tcw = Tcw.data(); prob.fixed = fixed.data();
    prob.corrected = corrected.data(); prob.noncorrected = noncorrected.data();
    prob.n_corrected = (int)(Sc.size() / 8); prob.n_noncorrected = (int)(Sn.size() / 8);
    prob.S_corrected = Sc.data(); prob.S_noncorrected = Sn.data();
    prob.n_edges = (int)edge_i.size(); prob.edge_i = edge_i.data(); prob.edge_j = edge_j.data(); prob.edge_kind = edge_kind.data();
    prob.n_points = (int)point_ref.size(); prob.Xw = Xw.data(); prob.point_ref = point_ref.data();
    prob.fix_scale = bFixScale;
    orbx_eg_options2 opt;
    opt.iterations = 20;                                         // :1096
    opt.solver = ORBX_EG_SOLVER_AUTO;                            // the dense solve's bytes either way; beyond 1536 free keyframes the envelope
    if (orbx_optimize_essential_graph2(orbx_adapter::Device(), &prob, &opt, TcwOut.data(), XwOut.data(), NULL, NULL, NULL) != ORBX_OK)
        throw runtime_error(string("Optimizer::OptimizeEssentialGraph: ") + orbx_last_error());   // ORBX_E_CAPACITY: a map beyond the limits

    unique_lock<mutex> lock(pMap->mMutexMapUpdate);
    for (size_t i = 0; i < vpKFs.size(); i++) {                   // :1101-1119
        const map<KeyFrame*,int>::const_iterator found = kfIndex.find(vpKFs[i]);
        if (found == kfIndex.end()) continue;
        const float *T = &TcwOut[16 * (size_t)found->second];
        cv::Mat Tiw(4, 4, CV_32F);                               // Converter::toCvSE3
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) Tiw.at<float>(r, c) = T[4 * r + c];
        vpKFs[i]->SetPose(Tiw);
    }
    for (size_t i = 0; i < vpMPs.size(); i++) {                   // :1122-1152
        const int ip = pointIndex[i];
        if (ip < 0) continue;
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        cv::Mat pos(3, 1, CV_32F);                               // Converter::toCvMat(eigCorrectedP3Dw)
        for (int k = 0; k < 3; k++) pos.at<float>(k) = XwOut[3 * (size_t)ip + k];
        pMP->SetWorldPos(pos);
        pMP->UpdateNormalAndDepth();
    }
}

} // namespace ORB_SLAM2
