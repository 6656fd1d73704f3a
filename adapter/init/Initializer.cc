// adapter/init/Initializer.cc -- ORB_SLAM2::Initializer with Initialize on the device (adapter/init/Initializer.h): the gather of the
// keypoints, mvMatches12 and the draw of mvSets as the reference writes them (src/Initializer.cc:52-111), then ONE
// orbx_mono_init_initialize call and the filling of the reference's outputs.
#include "Initializer.h"

#include <stdexcept>
#include <string>
#include <string.h>

#include <orbx.h>

#include "orbx_device.h"

#include "Thirdparty/DBoW2/DUtils/Random.h"

namespace ORB_SLAM2
{

static void GatherXY(const std::vector<cv::KeyPoint> &vKeys, std::vector<float> &xy)
{
    xy.resize(2 * vKeys.size());
    for (size_t i = 0; i < vKeys.size(); i++) { xy[2 * i] = vKeys[i].pt.x; xy[2 * i + 1] = vKeys[i].pt.y; }
}

Initializer::Initializer(const Frame &ReferenceFrame, float sigma, int iterations) : mSigma(sigma), mMaxIterations(iterations)
{
    GatherXY(ReferenceFrame.mvKeysUn, mXY1);
    const cv::Mat &K = ReferenceFrame.mK;
    mK[0] = K.at<float>(0, 0); mK[1] = K.at<float>(1, 1); mK[2] = K.at<float>(0, 2); mK[3] = K.at<float>(1, 2);
    memset(mLast, 0, sizeof mLast);
    memset(mLastRt, 0, sizeof mLastRt);
}

bool Initializer::Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                             std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated)
{
    const size_t n1 = mXY1.size() / 2;
    memset(mLast, 0, sizeof mLast);
    memset(mLastRt, 0, sizeof mLastRt);

    // mvMatches12 (:60-75): the matched keypoints in rising index of frame 1
    mMatches.clear();
    for (size_t i = 0; i < vMatches12.size() && i < n1; i++)
        if (vMatches12[i] >= 0) { mMatches.push_back((int32_t)i); mMatches.push_back(vMatches12[i]); }
    const int N = (int)(mMatches.size() / 2);
    if (N < 8) return false;     // the reference draws eight indices from a list of N

    // mvSets (:79-111): per row eight draws from the indices that are left, the drawn one replaced by the last; every row starts from the
    // full list.  All rows are drawn before anything is evaluated, as in the reference, so the random stream is the reference's.
    DUtils::Random::SeedRandOnce(0);
    mvSets.assign((size_t)mMaxIterations, std::vector<size_t>(8, 0));
    mSamples.resize(8 * (size_t)mMaxIterations);
    std::vector<size_t> left;
    for (int it = 0; it < mMaxIterations; it++) {
        left.resize((size_t)N);
        for (int i = 0; i < N; i++) left[i] = (size_t)i;
        for (int j = 0; j < 8; j++) {
            const int at = DUtils::Random::RandomInt(0, (int)left.size() - 1);
            mvSets[it][j] = left[at];
            mSamples[8 * (size_t)it + j] = (int32_t)left[at];
            left[at] = left.back();
            left.pop_back();
        }
    }

    // everything else is one call
    GatherXY(CurrentFrame.mvKeysUn, mXY2);
    mP3D.assign(3 * n1, 0.0f);
    mTriangulated.assign(n1, 0);
    orbx_mono_init_job job;
    memset(&job, 0, sizeof job);
    job.n1 = (int)n1; job.n2 = (int)(mXY2.size() / 2);
    job.xy1 = mXY1.data(); job.xy2 = mXY2.data();
    job.n = N; job.matches = mMatches.data();
    job.sigma = mSigma;
    memcpy(job.K, mK, sizeof job.K);
    job.min_parallax = 1.0; job.min_triangulated = 50;     // what Initialize passes to ReconstructH / ReconstructF (:139, :142)
    job.n_hyp = mMaxIterations; job.samples = mSamples.data();
    orbx_mono_init_result res;
    memset(&res, 0, sizeof res);
    res.P3D = mP3D.data(); res.triangulated = mTriangulated.data();
    if (orbx_mono_init_initialize(orbx_adapter::Device(), &job, &res) != ORBX_OK)
        throw std::runtime_error(std::string("Initializer::Initialize: ") + orbx_last_error());

    mLast[0] = res.ok; mLast[1] = res.model; mLast[2] = res.best_h; mLast[3] = res.best_f; mLast[4] = res.winner;
    memcpy(mLastRt, res.R21, sizeof res.R21); memcpy(mLastRt + 9, res.t21, sizeof res.t21); mLastRt[12] = res.parallax;
    if (!res.ok) return false;

    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R21.at<float>(r, c) = res.R21[3 * r + c];
        t21.at<float>(r) = res.t21[r];
    }
    vP3D.resize(n1);
    vbTriangulated.assign(n1, false);
    for (size_t i = 0; i < n1; i++) {
        vP3D[i] = cv::Point3f(mP3D[3 * i], mP3D[3 * i + 1], mP3D[3 * i + 2]);
        vbTriangulated[i] = mTriangulated[i] != 0;
    }
    return true;
}

#ifdef ORBX_ADAPTER_CAPTURE
Initializer::Capture Initializer::capture() const
{
    Capture c;
    c.xy1 = &mXY1; c.xy2 = &mXY2; c.P3D = &mP3D; c.matches = &mMatches; c.samples = &mSamples; c.triangulated = &mTriangulated;
    c.sets = &mvSets;
    memcpy(c.K, mK, sizeof c.K);
    c.sigma = mSigma;
    c.ok = mLast[0]; c.model = mLast[1]; c.best_h = mLast[2]; c.best_f = mLast[3]; c.winner = mLast[4];
    memcpy(c.R21, mLastRt, sizeof c.R21); memcpy(c.t21, mLastRt + 9, sizeof c.t21); c.parallax = mLastRt[12];
    return c;
}
#endif

} //namespace ORB_SLAM
