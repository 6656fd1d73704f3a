// adapter/orbx_batch.h -- the vocabulary-guided searches in the form the GPU wins with: keyframes RESIDENT in HBM and the loops the
// reference runs these searches in as ONE call each.
//
//   reference loop                                                            one call here
//   LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:241-309             SearchForTriangulationBatch(cur, neighbours, F12s, ...)
//     for each of 10-20 neighbour keyframes: ComputeF12 + matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false)
//   LoopClosing::ComputeSim3, src/LoopClosing.cc:293-323                      SearchByBoWBatch(cur, candidates, ...)
//     for each loop candidate: matcher.SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i])
//   LoopClosing::ComputeSim3, src/LoopClosing.cc:343-400                      Sim3SolverBatch(vpSim3Solvers)   (adapter/sim3/Sim3Solver.h)
//     for each loop candidate, five at a time: pSolver->iterate(5, ...) -- every hypothesis of every solver in one launch, then replayed
//   Tracking::Relocalization, src/Tracking.cc:1661-1682                       SearchByBoWBatch(candidates, mCurrentFrame, ...)
//     for each relocalisation candidate: matcher.SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i])
//
// A single SearchByBoW / SearchForTriangulation call costs 20-31 us on the GPU (one launch + one PCIe round trip) against 11-16 us on
// a host core; twenty pairs in one call cost 3-4.5 us per pair, this file's work included (matchers).  What makes the batch cheap is that a keyframe's
// descriptors, FeatureVector and undistorted keypoints never change once it exists (src/KeyFrame.cc:29-60): KeyFrameCache keeps them
// in HBM (orbx_kf), and a call moves only the map-point flags, the node intersection and the results.
//
// The reference's include/ORBmatcher.h is not touched: mfNNratio / mbCheckOrientation are protected there, so these free functions
// take the two constructor arguments of the `ORBmatcher matcher(ratio, checkOri)` the loop declares (0.6 / false in
// CreateNewMapPoints, 0.75 / true in ComputeSim3 and Relocalization).
#ifndef ORBX_ADAPTER_BATCH_H
#define ORBX_ADAPTER_BATCH_H

#include <stddef.h>
#include <stdint.h>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

#include <orbx.h>

namespace ORB_SLAM2
{
class KeyFrame;
class Frame;
class MapPoint;
}

namespace orbx_adapter
{

// One orbx_kf per KeyFrame*: made on first use from mDescriptors / mFeatVec / mvKeysUn / mvuRight (KeyFrame::ComputeBoW must have
// run: src/LocalMapping.cc:118, :246 guarantee it before any of the three loops), dropped when the keyframe goes away.
// Hook: call KeyFrameCache::instance().drop(this) from KeyFrame::SetBadFlag (src/KeyFrame.cc:459-503, after mbBad = true).
// Thread-safe (Tracking, LocalMapping and LoopClosing all match concurrently); the orbx_kf objects are immutable.
class KeyFrameCache
{
public:
    static KeyFrameCache &instance();
    const orbx_kf *get(ORB_SLAM2::KeyFrame *pKF);            // creates the resident copy if there is none yet; throws on failure
    const orbx_kf *find(const ORB_SLAM2::KeyFrame *pKF);     // NULL when pKF is not resident
    void drop(const ORB_SLAM2::KeyFrame *pKF);
    void clear();
    size_t size();
    ~KeyFrameCache();

private:
    KeyFrameCache() {}
    KeyFrameCache(const KeyFrameCache &);
    KeyFrameCache &operator=(const KeyFrameCache &);
    std::mutex mMutex;
    std::map<const ORB_SLAM2::KeyFrame *, orbx_kf *> mKFs;
};

// ---- resident keyframes for the projection searches whose target is a keyframe: both Fuse overloads, SearchBySim3 and the Sim3
// SearchByProjection (adapter/ORBmatcher_fuse.cc).  One orbx_frame per KeyFrame* -- mvKeysUn, mvuRight, mDescriptors, the keyframe's image
// bounds and the 64x48 grid in HBM -- so that a search moves only the projected points.  Opt-in like KeyFrameCache: get() makes the
// resident copy (hooks: the end of the KeyFrame constructor, src/KeyFrame.cc:29-60, or the first use of a target in
// LocalMapping::SearchInNeighbors, src/LocalMapping.cc:515-599; drop() from KeyFrame::SetBadFlag); the four adaptors use a resident
// keyframe only when find() returns one and take the host-pointer path otherwise, so a program that registers nothing behaves as before.
// A KeyFrame* can be recycled by the allocator, so the address alone proves nothing: every entry keeps a host shadow of what it uploaded
// (N, the bounds, the mvKeysUn records, mvuRight, the descriptor bytes), get() and find() compare it with memcmp (a few microseconds at
// 1000 features) and rebuild the resident copy on any difference.  Thread-safe; a FrameRef keeps its orbx_frame alive while another
// thread drops or rebuilds the entry, and the searches only read the handle (include/orbx.h).
typedef std::shared_ptr<const orbx_frame> FrameRef;
class KeyFrameFrames
{
public:
    static KeyFrameFrames &instance();
    FrameRef get(ORB_SLAM2::KeyFrame *pKF);      // the resident copy, made (or rebuilt) if need be; throws on failure
    FrameRef find(ORB_SLAM2::KeyFrame *pKF);     // empty when pKF is not registered; a stale entry is rebuilt
    void drop(const ORB_SLAM2::KeyFrame *pKF);
    void clear();
    size_t size();
    void stats(int *creates, int *hits);         // resident copies made (rebuilds included), look-ups served by an existing one
    ~KeyFrameFrames();

private:
    struct Entry {
        FrameRef frame;
        int device, n;
        float bounds[4];
        std::vector<cv::KeyPoint> keys;
        std::vector<float> u_right;
        std::vector<uint8_t> desc;
    };
    KeyFrameFrames() : mCreates(0), mHits(0) {}
    KeyFrameFrames(const KeyFrameFrames &);
    KeyFrameFrames &operator=(const KeyFrameFrames &);
    FrameRef lookup(ORB_SLAM2::KeyFrame *pKF, bool create);
    std::mutex mMutex;
    std::map<const ORB_SLAM2::KeyFrame *, Entry> mKFs;
    int mCreates, mHits;
};

// The first loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:549-554) as one call: afterwards the map is exactly what
//     for (t = 0; t < vpTargetKFs.size(); t++) vnFused[t] = matcher.Fuse(vpTargetKFs[t], vpMapPoints, th);
// leaves, and vnFused holds its return values.  All (target, point) pairs are projected and searched in ONE
// orbx_frame_window_best_batch with the descriptors as they are at entry (the targets become resident through KeyFrameFrames::get);
// the surgery then walks the targets in order.  What a target's surgery can change for the targets behind it: a point goes bad or into
// a keyframe (validity only goes from valid to invalid; re-checked before every Replace / AddObservation, as the single Fuse does), and
// a Replace ends in the survivor's ComputeDistinctiveDescriptors (src/MapPoint.cc:190-229), so a surviving point's descriptor can
// differ when the next target is searched.  World position, normal and distance range do not change inside the loop.  So before target
// t's surgery every still-valid point's current descriptor bytes are compared with the bytes uploaded, and the points that differ are
// searched again against target t alone (one orbx_frame_window_best; no call when none differs).
// Cost (profiles/r08_kf_fuse.txt): the device part is 5 us per target against 38-40 us for a single resident call, but every pair is
// projected on the host at entry -- also pairs whose point an earlier target's surgery would have made bad before the loop reached them.
// Where most points die early in the loop, the loop of single resident Fuse calls is the cheaper form.
// The second half of SearchInNeighbors (:579) is a single Fuse into the current keyframe: register it and Fuse() takes the resident
// call.  LoopClosing::SearchAndFuse's loop (src/LoopClosing.cc:732-759) is NOT covered: its Fuse overload defers the replacements to
// the caller, which takes the map mutex per keyframe.
void FuseBatch(const std::vector<ORB_SLAM2::KeyFrame *> &vpTargetKFs, const std::vector<ORB_SLAM2::MapPoint *> &vpMapPoints,
               std::vector<int> &vnFused, float th = 3.0f);
// the calling thread's counts: batch launches made by FuseBatch, points it searched again because their descriptor had changed
void FuseBatchStats(int *launches, int *researched);

// src/LocalMapping.cc:241-309 as one call: vF12[i] = ComputeF12(pKF1, vpKF2[i]) (3x3 CV_32F), vvMatchedPairs[i] = what
// matcher.SearchForTriangulation(pKF1, vpKF2[i], vF12[i], vMatchedIndices, bOnlyStereo) would have returned.  Returns the total.
// "Would have returned" with the map-point flags as they are AT ENTRY: the reference's loop creates points between two searches, and a
// feature of pKF1 that got one is skipped by the later searches (src/ORBmatcher.cc:750-751), so the lists here can name a feature of pKF1
// at several neighbours.  A caller that triangulates them must keep, per idx1, only the first neighbour whose tests pass --
// adapter/triangulate/CreateNewMapPoints.h does the search and the triangulation with that rule.
int SearchForTriangulationBatch(ORB_SLAM2::KeyFrame *pKF1, const std::vector<ORB_SLAM2::KeyFrame *> &vpKF2, const std::vector<cv::Mat> &vF12,
                                std::vector<std::vector<std::pair<size_t, size_t> > > &vvMatchedPairs, bool bOnlyStereo,
                                float nnratio = 0.6f, bool checkOri = false);

// src/LoopClosing.cc:293-323 as one call: vvpMatches12[i] and vnMatches[i] = what matcher.SearchByBoW(pKF1, vpKF2[i], vvpMatches12[i])
// would have produced / returned.
void SearchByBoWBatch(ORB_SLAM2::KeyFrame *pKF1, const std::vector<ORB_SLAM2::KeyFrame *> &vpKF2,
                      std::vector<std::vector<ORB_SLAM2::MapPoint *> > &vvpMatches12, std::vector<int> &vnMatches,
                      float nnratio = 0.75f, bool checkOri = true);

// src/Tracking.cc:1661-1682 as one call: vvpMapPointMatches[i] and vnMatches[i] = what matcher.SearchByBoW(vpKFs[i], F,
// vvpMapPointMatches[i]) would have produced / returned.  Keyframes resident, the frame as host pointers (it lives one frame time).
void SearchByBoWBatch(const std::vector<ORB_SLAM2::KeyFrame *> &vpKFs, ORB_SLAM2::Frame &F,
                      std::vector<std::vector<ORB_SLAM2::MapPoint *> > &vvpMapPointMatches, std::vector<int> &vnMatches,
                      float nnratio = 0.75f, bool checkOri = true);

// flag arrays the resident searches take per call (exactly what adapter/ORBmatcher_bow.cc hands the host-pointer entries)
void GoodPointFlags(ORB_SLAM2::KeyFrame *pKF, std::vector<ORB_SLAM2::MapPoint *> &vpMapPoints, std::vector<uint8_t> &flag);   // SearchByBoW: non-bad MapPoint
void HasPointFlags(ORB_SLAM2::KeyFrame *pKF, std::vector<uint8_t> &flag);                                                      // SearchForTriangulation: any MapPoint
// epipole of camera 1 in image 2 (src/ORBmatcher.cc:712-718)
void Epipole(ORB_SLAM2::KeyFrame *pKF1, ORB_SLAM2::KeyFrame *pKF2, float &ex, float &ey);

} // namespace orbx_adapter

#endif
