// adapter/triangulate/CreateNewMapPoints.h -- the two halves of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:237-513)
// as two device calls with nothing but the pair lists in between: SearchForTriangulationBatch (adapter/orbx_batch.h) and the
// triangulation of every pair (orbx_frame_triangulate, or orbx_triangulate_pairs for keyframes that are not resident).
//
// THE ORDER RULE.  The reference's loop creates points neighbour by neighbour, and a point created for feature idx1 of the current keyframe
// makes SearchForTriangulation skip idx1 at every later neighbour (src/ORBmatcher.cc:750-751).  SearchForTriangulationBatch searches all
// neighbours with the flags as they are at entry, so a caller that triangulated its lists one by one would create duplicates.  The device
// call keeps, per idx1, only the pair of the FIRST neighbour whose tests pass; `out` is therefore exactly what the loop would have
// created, in the loop's order.  This holds for checkOri == false, which is what CreateNewMapPoints passes (with the orientation
// histogram a dropped row changes which rows survive).
//
// What stays in the caller: the baseline test at :278-300 and CheckNewKeyFrames (:273), in the loop that collects vpKF2 and vF12 -- the
// caller hands over only the neighbours that passed -- and :495-510 (new MapPoint, AddObservation, AddMapPoint,
// ComputeDistinctiveDescriptors, UpdateNormalAndDepth, Map::AddMapPoint, mlpRecentAddedMapPoints) over `out`.
// Its own sub-directory, like adapter/localmap/ and adapter/pose/: it needs KeyFrame members (mvKeys, mvDepth, mb, invfx, invfy) the
// stand-ins of the other adaptors' tests lack.
#ifndef ORBX_ADAPTER_CREATE_NEW_MAP_POINTS_H
#define ORBX_ADAPTER_CREATE_NEW_MAP_POINTS_H

#include <stddef.h>
#include <stdint.h>
#include <vector>

#include <opencv2/core/core.hpp>

#include <orbx.h>

namespace ORB_SLAM2
{
class KeyFrame;
}

namespace orbx_adapter
{

struct NewPoint {
    size_t neighbour;    // index into vpKF2
    size_t idx1, idx2;   // the feature of pKF1 and of vpKF2[neighbour]
    cv::Mat x3D;         // 3 x 1 CV_32F, what the loop hands to `new MapPoint` (:495)
};

// vF12[i] = ComputeF12(pKF1, vpKF2[i]); ratioFactor = 1.5f * pKF1->mfScaleFactor (:265).  Runs SearchForTriangulationBatch (bOnlyStereo =
// false, checkOri = false), then triangulates on the keyframes' resident copies when ALL of them are registered with KeyFrameFrames
// (adapter/orbx_batch.h) -- mvDepth and the raw positions are attached to a resident copy on its first use here -- and from host pointers
// otherwise.  Returns out.size(); throws std::runtime_error when the library refuses.
int CreateNewMapPointsBatch(ORB_SLAM2::KeyFrame *pKF1, const std::vector<ORB_SLAM2::KeyFrame *> &vpKF2, const std::vector<cv::Mat> &vF12,
                            std::vector<NewPoint> &out, float ratioFactor);

// a keyframe's arrays behind an orbx_tri_feats (host-pointer call) or an orbx_frame_set_depth: mvKeysUn, mvuRight, mvDepth (empty when
// the keyframe keeps none: a monocular map), mvKeys
struct TriKeyFrame {
    std::vector<float> x, y, u_right, depth, raw_x, raw_y;
    std::vector<int32_t> octave;
    explicit TriKeyFrame(ORB_SLAM2::KeyFrame *pKF = NULL);
    orbx_tri_feats feats() const;
};

#ifdef ORBX_ADAPTER_CAPTURE
// test hook (tests/adapter_triangulate_driver.cc): what the last call handed to the ABI.  Not compiled into a production build.
struct TriCapture {
    bool resident;
    std::vector<TriKeyFrame> kfs;        // pKF1, then the neighbours
    std::vector<orbx_tri_view> views;    // likewise
    std::vector<int32_t> pairs; std::vector<int> npairs; int cap;
    std::vector<float> scale_factors, level_sigma2;
    float ratio_factor;
    std::vector<uint8_t> status; std::vector<float> x3d; int n_new;
};
TriCapture &tri_capture();
#endif

} // namespace orbx_adapter

#endif
