// adapter/pose/PoseOptimization.cc -- int ORB_SLAM2::Optimizer::PoseOptimization(Frame *pFrame) (reference src/Optimizer.cc:286-513) on the
// device: the gather of :326-420 under MapPoint::mGlobalMutex, ONE call of orbx_pose_optimize (one upload, one launch, one download:
// the four rounds of Levenberg iterations and the classifications between them run in the kernel), then mvbOutlier, SetPose and the return
// value.  It replaces that one function only: the rest of src/Optimizer.cc -- the bundle adjustments, the essential graph, OptimizeSim3 --
// has adaptors of its own (adapter/lba/, adapter/ba/, adapter/essential/, adapter/sim3opt/).  Its own sub-directory, like adapter/localmap/: it needs Optimizer.h and Frame::SetPose.
#include "Optimizer.h"

#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_device.h"

namespace ORB_SLAM2
{

int Optimizer::PoseOptimization(Frame *pFrame)
{
    const int N = pFrame->N;
    std::vector<float> x(N), y(N), ur(N), isig(N), Xw(3 * (size_t)N);
    std::vector<unsigned char> has(N, 0), outlier(N, 0);
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);
        for (int i = 0; i < N; i++) {
            MapPoint *pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            const cv::KeyPoint &kpUn = pFrame->mvKeysUn[i];
            has[i] = 1;
            pFrame->mvbOutlier[i] = false;                       // :338, :381
            x[i] = kpUn.pt.x; y[i] = kpUn.pt.y; ur[i] = pFrame->mvuRight[i];
            isig[i] = pFrame->mvInvLevelSigma2[kpUn.octave];
            const cv::Mat P = pMP->GetWorldPos();
            Xw[3 * (size_t)i] = P.at<float>(0); Xw[3 * (size_t)i + 1] = P.at<float>(1); Xw[3 * (size_t)i + 2] = P.at<float>(2);
        }
    }
    orbx_pose_obs obs;
    obs.n = N;
    obs.x = x.data(); obs.y = y.data(); obs.u_right = ur.data(); obs.inv_sigma2 = isig.data(); obs.Xw = Xw.data(); obs.has_point = has.data();
    const float cam[5] = { pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy, pFrame->mbf };
    float Tcw[16], Tout[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) Tcw[4 * r + c] = pFrame->mTcw.at<float>(r, c);
    int nInliers = 0;
    orbx_pose_report rep;
    if (orbx_pose_optimize(orbx_adapter::Device(), &obs, cam, Tcw, Tout, outlier.data(), &nInliers, &rep) != ORBX_OK)
        throw std::runtime_error(std::string("Optimizer::PoseOptimization: ") + orbx_last_error());
    if (rep.n_corr < 3)                                          // :423-424: no SetPose, the flags stay false
        return 0;
    for (int i = 0; i < N; i++)
        if (has[i]) pFrame->mvbOutlier[i] = outlier[i] != 0;
    cv::Mat pose(4, 4, CV_32F);                                  // Converter::toCvMat(SE3quat_recov)
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = Tout[4 * r + c];
    pFrame->SetPose(pose);
    return nInliers;                                             // nInitialCorrespondences - nBad
}

} // namespace ORB_SLAM2
