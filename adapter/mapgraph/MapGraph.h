// adapter/mapgraph/MapGraph.h -- the observation graph resident on the device, and the three walks of the reference that run on it.
//
// LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:704-775), the counting loop of KeyFrame::UpdateConnections
// (src/KeyFrame.cc:303-338) and the voting loop of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1515-1538) all walk
// KeyFrame::mvpMapPoints against MapPoint::mObservations.  MapGraph keeps both in an orbx_mapgraph, a slot per KeyFrame* and per MapPoint*,
// fed by hooks in the reference's mutators: a hook only queues a small record under a mutex, and the queue is sent, in order and in
// batches, before the next query.
//
// Hooks in the reference; G = orbx_adapter::MapGraph::instance():
//   KeyFrame::KeyFrame (end)                 G.OnNewKeyFrame(this);
//   KeyFrame::AddMapPoint                    G.OnSetMatch(this, idx, pMP);
//   KeyFrame::EraseMapPointMatch (both)      G.OnSetMatch(this, idx, NULL);        (the MapPoint* form: idx = pMP->GetIndexInKeyFrame(this), if >= 0)
//   KeyFrame::ReplaceMapPointMatch           G.OnSetMatch(this, idx, pMP);
//   KeyFrame::SetBadFlag                     G.OnKeyFrameBad(this);                (behind the mnId == 0 / mbNotErase returns, :500)
//   MapPoint::AddObservation (top)           G.OnAddObservation(this, pKF, idx);
//   MapPoint::EraseObservation (top)         G.OnEraseObservation(this, pKF);
//   MapPoint::SetBadFlag, MapPoint::Replace  G.OnPointBad(this);                   (top; Replace's own Add / Replace / Erase calls follow through their hooks)
//   Map::clear                               G.OnMapClear();
//   include/KeyFrame.h                       bool GetNotErase();                   (mbNotErase under mMutexConnections)
// Identity is the pair (address, mnId): an object that turns up at a known address with another mnId is a new object, and the old one's
// slot is given up first (first finding: Map::clear deletes without SetBadFlag).
#ifndef ORBX_ADAPTER_MAPGRAPH_H
#define ORBX_ADAPTER_MAPGRAPH_H

#include <stddef.h>
#include <stdint.h>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include <orbx.h>

namespace ORB_SLAM2
{
class Frame;
class KeyFrame;
class MapPoint;
}

namespace orbx_adapter
{

struct RefreshStats;

class MapGraph
{
public:
    // the process-wide graph (ORB-SLAM2 has one Map).  Capacities from the environment or: ORBX_MAPGRAPH_KEYFRAMES 4096, ORBX_MAPGRAPH_FEATURES
    // 4096, ORBX_MAPGRAPH_POINTS 262144, ORBX_MAPGRAPH_OBS 256 -- 350 MiB on the device and as much on the host; fixed when the first
    // flush creates the graph on orbx_adapter::Device()
    static MapGraph &instance();
    MapGraph(int max_keyframes, int max_features, int max_points, int max_obs);
    ~MapGraph();

    void OnNewKeyFrame(ORB_SLAM2::KeyFrame *pKF);
    void OnSetMatch(ORB_SLAM2::KeyFrame *pKF, size_t idx, ORB_SLAM2::MapPoint *pMP);
    void OnKeyFrameBad(ORB_SLAM2::KeyFrame *pKF);
    void OnAddObservation(ORB_SLAM2::MapPoint *pMP, ORB_SLAM2::KeyFrame *pKF, size_t idx);
    void OnEraseObservation(ORB_SLAM2::MapPoint *pMP, ORB_SLAM2::KeyFrame *pKF);
    void OnPointBad(ORB_SLAM2::MapPoint *pMP);
    void OnMapClear();

    // the queue sent, in order: consecutive records of one kind travel as one batch
    void Flush();
    // LocalMapping::KeyFrameCulling's loop over `local` (mnId == 0 and keyframes without a slot left out by the caller): flag[j] = 0 keep, 1 culled
    // (the graph has erased it and its bad points already), 2 culled but mbNotErase
    void Cull(const std::vector<ORB_SLAM2::KeyFrame *> &local, bool monocular, std::vector<unsigned char> &flag);
    bool Knows(ORB_SLAM2::KeyFrame *pKF);

    // tests, tools
    int keyframes();            // keyframes that hold a slot
    int points();               // point slots handed out since the last Map::clear
    size_t queued();
    long batches_sent();        // ABI edit calls so far
    long echoes_dropped();      // hook calls recognised as already applied

    // on this thread, hooks are dropped while one of these lives: KeyFrameCulling holds one round the SetBadFlag calls whose map-point
    // part the graph has applied itself
    struct EchoScope { EchoScope(); ~EchoScope(); };

private:
    friend void CovisibilityCounts(ORB_SLAM2::KeyFrame *, std::map<ORB_SLAM2::KeyFrame *, int> &);
    friend void VoteLocalKeyFrames(ORB_SLAM2::Frame &, std::map<ORB_SLAM2::KeyFrame *, int> &);
    friend RefreshStats RefreshMapPoints(const std::vector<ORB_SLAM2::MapPoint *> &, int);      // adapter/mappoint/MapPointRefresh.cc
    enum Kind { SET_KEYFRAME, SET_MATCH, ADD_OBS, ERASE_OBS, ERASE_POINT, ERASE_KEYFRAME, CLEAR };
    struct Rec { Kind kind; int32_t a, b, c; };     // SET_KEYFRAME: slot, index into attr_, n; SET_MATCH: kf, idx, point; ADD_OBS: point, kf, idx;
                                                    // ERASE_OBS: point, kf; ERASE_POINT: point; ERASE_KEYFRAME: kf
    struct Id { int slot; unsigned long id; };
    int kf_slot(ORB_SLAM2::KeyFrame *pKF);          // -1: unknown, or known under another mnId (then given up)
    int point_slot(ORB_SLAM2::MapPoint *pMP, bool make);
    void give_up_keyframe(ORB_SLAM2::KeyFrame *pKF, bool queue);
    bool echo();
    orbx_mapgraph *graph();
    void flush_locked();
    void check(int rc);

    std::mutex mu_;
    int max_kf_, max_feat_, max_points_, max_obs_;
    orbx_mapgraph *graph_;
    std::unordered_map<ORB_SLAM2::KeyFrame *, Id> kf_;
    std::unordered_map<ORB_SLAM2::MapPoint *, Id> pt_;
    std::vector<ORB_SLAM2::KeyFrame *> kf_of_slot_;    // the last keyframe of every slot, also behind its SetBadFlag, until the slot is used again
    std::vector<int> kf_free_;                         // first in, first out
    size_t kf_free_head_;
    int kf_high_, pt_high_;                            // a point slot is not used again before Map::clear: a stale match may still name it
    std::vector<unsigned char> pt_bad_;
    std::vector<Rec> queue_;
    std::vector<unsigned char> attr_;                  // octave | stereo | close of the queued new keyframes, 3 * n bytes each
    long batches_, echoes_;
};

// KFcounter of KeyFrame::UpdateConnections (src/KeyFrame.cc:305-338), filled from one orbx_mapgraph_covisibility call; the threshold, the
// maximum, the sort and the spanning tree stay the reference's text
void CovisibilityCounts(ORB_SLAM2::KeyFrame *pKF, std::map<ORB_SLAM2::KeyFrame *, int> &KFcounter);
// keyframeCounter of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1519-1538) from one orbx_mapgraph_vote call; a bad point's entry of
// F.mvpMapPoints is set to NULL as the reference does
void VoteLocalKeyFrames(ORB_SLAM2::Frame &F, std::map<ORB_SLAM2::KeyFrame *, int> &keyframeCounter);

} // namespace orbx_adapter

#endif
