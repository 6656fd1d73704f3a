// adapter/sim3opt/OptimizeSim3.cc -- int ORB_SLAM2::Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint *> &vpMatches1,
// g2o::Sim3 &g2oS12, const float th2, const bool bFixScale) (reference src/Optimizer.cc:1164-1365) on the device: the gather of :1205-1302
// under the reference's accessors, ONE call of orbx_sim3_optimize (one upload, one launch, one download: both rounds of Levenberg
// iterations and the classification after each run in the kernel), then vpMatches1[i] = NULL where the pair left, g2oS12 assigned only
// where the reference reaches :1362 (not on the early return of 0), and the return value.  With it LoopClosing::ComputeSim3 needs no g2o
// between its first search and its last, and LoopClosing does not change.  It replaces that one function only.  Its
// own sub-directory, like adapter/pose/.
#include "Optimizer.h"

#include <stdexcept>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_device.h"

namespace ORB_SLAM2
{

int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale)
{
    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    const float cam1[4] = { K1.at<float>(0, 0), K1.at<float>(1, 1), K1.at<float>(0, 2), K1.at<float>(1, 2) };
    const float cam2[4] = { K2.at<float>(0, 0), K2.at<float>(1, 1), K2.at<float>(0, 2), K2.at<float>(1, 2) };
    const cv::Mat R1w = pKF1->GetRotation();
    const cv::Mat t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation();
    const cv::Mat t2w = pKF2->GetTranslation();

    const int N = vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<float> P1c(3 * (size_t)N), P2c(3 * (size_t)N), x1(N), y1(N), w1(N), x2(N), y2(N), w2(N);
    std::vector<unsigned char> has(N, 0), inlier(N, 0);
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2 || pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;    // :1235-1260
        const cv::Mat P3D1c = R1w * pMP1->GetWorldPos() + t1w;                      // :1241-1242
        const cv::Mat P3D2c = R2w * pMP2->GetWorldPos() + t2w;                      // :1249-1250
        for (int k = 0; k < 3; k++) { P1c[3 * (size_t)i + k] = P3D1c.at<float>(k); P2c[3 * (size_t)i + k] = P3D2c.at<float>(k); }
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];
        x1[i] = kpUn1.pt.x; y1[i] = kpUn1.pt.y; w1[i] = pKF1->mvInvLevelSigma2[kpUn1.octave];
        x2[i] = kpUn2.pt.x; y2[i] = kpUn2.pt.y; w2[i] = pKF2->mvInvLevelSigma2[kpUn2.octave];
        has[i] = 1;
    }
    orbx_sim3opt_obs obs;
    obs.n = N;
    obs.has_pair = has.data(); obs.P1c = P1c.data(); obs.P2c = P2c.data();
    obs.x1 = x1.data(); obs.y1 = y1.data(); obs.inv_sigma2_1 = w1.data();
    obs.x2 = x2.data(); obs.y2 = y2.data(); obs.inv_sigma2_2 = w2.data();
    const Eigen::Quaterniond &r = g2oS12.rotation();
    const Eigen::Vector3d &t = g2oS12.translation();
    const double S12[8] = { r.x(), r.y(), r.z(), r.w(), t[0], t[1], t[2], g2oS12.scale() };
    double S12_out[8];
    int nIn = 0;
    orbx_sim3opt_report rep;
    if (orbx_sim3_optimize(orbx_adapter::Device(), &obs, cam1, cam2, S12, th2, bFixScale ? 1 : 0, S12_out, inlier.data(), &nIn, &rep) != ORBX_OK)
        throw std::runtime_error(std::string("Optimizer::OptimizeSim3: ") + orbx_last_error());
    for (int i = 0; i < N; i++)
        if (has[i] && !inlier[i]) vpMatches1[i] = static_cast<MapPoint *>(NULL);   // :1320, :1354 (also on the return of 0 at :1336)
    if (rep.rounds < 2)                                                            // :1335-1336: returned 0 before g2oS12 was assigned
        return 0;
    // Eigen's Quaterniond(w, x, y, z)
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(S12_out[3], S12_out[0], S12_out[1], S12_out[2]), Eigen::Vector3d(S12_out[4], S12_out[5], S12_out[6]), S12_out[7]);
    return nIn;
}

} // namespace ORB_SLAM2
