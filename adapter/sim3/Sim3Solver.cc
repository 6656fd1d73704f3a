// adapter/sim3/Sim3Solver.cc -- ORB_SLAM2::Sim3Solver with the hypotheses on the device (adapter/sim3/Sim3Solver.h): the gather of the
// reference's constructor (src/Sim3Solver.cc:37-113), the draw of the sample triples (:166-181), ONE orbx_sim3_hypotheses(_batch) call,
// and the state machine of Sim3Solver::iterate (:143-211) replayed over the table the call returns.
#include "Sim3Solver.h"

#include <algorithm>
#include <limits.h>
#include <math.h>
#include <stdexcept>
#include <string>
#include <string.h>

#include <orbx.h>

#include "MapPoint.h"
#include "orbx_device.h"

#include "Thirdparty/DBoW2/DUtils/Random.h"

namespace ORB_SLAM2
{

// what the reference's comparison `err < mvnMaxError[i]` sees: 9.210 * sigma2 went through a vector<size_t> (include/orbx.h, "size_t")
static float max_error(float sigma2) { return (float)(size_t)(9.210 * sigma2); }

static void intrinsics(const cv::Mat &K, float out[4])
{
    out[0] = K.at<float>(0, 0); out[1] = K.at<float>(1, 1); out[2] = K.at<float>(0, 2); out[3] = K.at<float>(1, 2);
}

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale)
    : N(0), mN1((int)vpMatched12.size()), mbFixScale(bFixScale), mnIterations(0), mnBestInliers(0)
{
    const std::vector<MapPoint *> own = pKF1->GetMapPointMatches();
    const cv::Mat R1 = pKF1->GetRotation(), t1 = pKF1->GetTranslation(), R2 = pKF2->GetRotation(), t2 = pKF2->GetTranslation();
    for (int i = 0; i < mN1; i++) {
        MapPoint *p1 = own[i], *p2 = vpMatched12[i];
        if (!p2 || !p1 || p1->isBad() || p2->isBad()) continue;
        const int k1 = p1->GetIndexInKeyFrame(pKF1), k2 = p2->GetIndexInKeyFrame(pKF2);
        if (k1 < 0 || k2 < 0) continue;
        mMaxErr1.push_back(max_error(pKF1->mvLevelSigma2[pKF1->mvKeysUn[k1].octave]));
        mMaxErr2.push_back(max_error(pKF2->mvLevelSigma2[pKF2->mvKeysUn[k2].octave]));
        mIndex1.push_back((size_t)i);
        const cv::Mat c1 = R1 * p1->GetWorldPos() + t1, c2 = R2 * p2->GetWorldPos() + t2;
        for (int r = 0; r < 3; r++) { mX1.push_back(c1.at<float>(r)); mX2.push_back(c2.at<float>(r)); }
    }
    intrinsics(pKF1->mK, mK1);
    intrinsics(pKF2->mK, mK2);
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    mProb = probability;
    mMinInliers = minInliers;
    N = (int)mIndex1.size();
    int its = 1;
    if (minInliers != N) {
        const float epsilon = (float)minInliers / N;
        const double x = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        // fewer correspondences than minInliers: the logarithm is NaN and iterate() never loops; the count is then 1
        its = x == x ? (int)std::max((double)INT_MIN, std::min((double)INT_MAX, x)) : INT_MIN;
    }
    mMaxIts = std::max(1, std::min(its, maxIterations));
    mnIterations = 0;
    mTable.ready = false;     // another iteration count: triples are drawn and evaluated again
}

bool Sim3Solver::NeedsTable() const { return !mTable.ready && N >= mMinInliers && N >= 3; }

void Sim3Solver::Draw()
{
    const size_t its = (size_t)mMaxIts, words = ((size_t)N + 63) / 64;
    mTable.samples.resize(3 * its);
    // every hypothesis draws from the full list 0 .. N-1, the drawn index replaced by the last one that is left (:166-181).  The
    // reference copies the list per hypothesis; undoing the three replacements gives the same list without the copy.
    std::vector<int32_t> left((size_t)N);
    for (int i = 0; i < N; i++) left[i] = i;
    for (size_t h = 0; h < its; h++) {
        int at[3];
        int32_t drawn[3], last[3];
        for (int k = 0; k < 3; k++) {
            at[k] = DUtils::Random::RandomInt(0, (int)left.size() - 1);
            drawn[k] = left[at[k]]; last[k] = left.back();
            mTable.samples[3 * h + k] = drawn[k];
            left[at[k]] = last[k];
            left.pop_back();
        }
        for (int k = 2; k >= 0; k--) { left.push_back(last[k]); left[at[k]] = drawn[k]; }
    }
    mTable.count.assign(its, 0);
    mTable.srt.assign(13 * its, 0.f);
    mTable.bits.assign(words * its, 0);
}

cv::Mat Sim3Solver::Pose(const float *srt) const
{
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T.at<float>(r, c) = (float)((double)srt[0] * (double)srt[1 + 3 * r + c]);   // ms12i * mR12i
        T.at<float>(r, 3) = srt[10 + r];
        T.at<float>(3, r) = 0.f;
    }
    T.at<float>(3, 3) = 1.f;
    return T;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers.assign((size_t)mN1, false);
    nInliers = 0;
    if (N < mMinInliers || N < 3) {
        bNoMore = true;
        return cv::Mat();
    }
    if (!mTable.ready) {
        std::vector<Sim3Solver *> me(1, this);
        orbx_adapter::Sim3SolverBatch(me);
    }
    const size_t words = ((size_t)N + 63) / 64;
    for (int done = 0; mnIterations < mMaxIts && done < nIterations; done++) {
        const size_t h = (size_t)mnIterations++;
        const int count = mTable.count[h];
        if (count < mnBestInliers) continue;
        mnBestInliers = count;                  // >=: a later tie replaces the best
        mBest.assign(&mTable.srt[13 * h], &mTable.srt[13 * h] + 13);
        if (count <= mMinInliers) continue;     // strictly more than minInliers returns, and only from a new best
        const uint64_t *bits = &mTable.bits[words * h];
        for (int i = 0; i < N; i++)
            if ((bits[i >> 6] >> (i & 63)) & 1) vbInliers[mIndex1[i]] = true;
        nInliers = count;
        return Pose(&mBest[0]);
    }
    bNoMore = mnIterations >= mMaxIts;
    return cv::Mat();
}

cv::Mat Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers)
{
    bool more;
    return iterate(mMaxIts, more, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation()
{
    if (mBest.empty()) return cv::Mat();
    cv::Mat R(3, 3, CV_32F);
    for (int k = 0; k < 9; k++) R.at<float>(k / 3, k % 3) = mBest[1 + k];
    return R;
}

cv::Mat Sim3Solver::GetEstimatedTranslation()
{
    if (mBest.empty()) return cv::Mat();
    cv::Mat t(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) t.at<float>(k) = mBest[10 + k];
    return t;
}

float Sim3Solver::GetEstimatedScale() { return mBest.empty() ? 0.f : mBest[0]; }

#ifdef ORBX_ADAPTER_CAPTURE
Sim3Solver::Capture Sim3Solver::capture() const
{
    Capture c;
    c.N = N; c.mN1 = mN1; c.max_its = mMaxIts; c.fix_scale = mbFixScale ? 1 : 0;
    c.X1 = &mX1; c.X2 = &mX2; c.max_err1 = &mMaxErr1; c.max_err2 = &mMaxErr2;
    c.K1 = mK1; c.K2 = mK2;
    c.indices1 = &mIndex1;
    c.samples = &mTable.samples; c.n_inliers = &mTable.count; c.srt = &mTable.srt; c.bits = &mTable.bits;
    return c;
}
#endif

} // namespace ORB_SLAM2

namespace orbx_adapter
{

void Sim3SolverBatch(std::vector<ORB_SLAM2::Sim3Solver *> &vpSolvers)
{
    std::vector<orbx_sim3_job> jobs;
    std::vector<ORB_SLAM2::Sim3Solver *> taken;
    for (size_t i = 0; i < vpSolvers.size(); i++) {
        ORB_SLAM2::Sim3Solver *p = vpSolvers[i];
        if (!p || !p->NeedsTable() || std::find(taken.begin(), taken.end(), p) != taken.end()) continue;
        taken.push_back(p);
        p->Draw();
        const size_t words = ((size_t)p->N + 63) / 64;
        for (int first = 0; first < p->mMaxIts; first += 1024) {     // a call takes 1024 hypotheses per job
            orbx_sim3_job j;
            memset(&j, 0, sizeof j);
            j.n = p->N;
            j.X1 = &p->mX1[0]; j.X2 = &p->mX2[0]; j.max_err1 = &p->mMaxErr1[0]; j.max_err2 = &p->mMaxErr2[0];
            memcpy(j.K1, p->mK1, sizeof j.K1); memcpy(j.K2, p->mK2, sizeof j.K2);
            j.fix_scale = p->mbFixScale ? 1 : 0;
            j.n_hyp = std::min(1024, p->mMaxIts - first);
            j.samples = &p->mTable.samples[3 * (size_t)first];
            j.n_inliers = &p->mTable.count[first]; j.srt = &p->mTable.srt[13 * (size_t)first]; j.inlier_bits = &p->mTable.bits[words * (size_t)first];
            jobs.push_back(j);
        }
    }
    for (size_t at = 0; at < jobs.size(); at += 64) {                 // ... and 64 jobs
        const int nj = (int)std::min((size_t)64, jobs.size() - at);
        const int rc = nj == 1 ? orbx_sim3_hypotheses(Device(), &jobs[at]) : orbx_sim3_hypotheses_batch(Device(), &jobs[at], nj);
        if (rc != ORBX_OK) throw std::runtime_error(std::string("Sim3Solver: ") + orbx_last_error());
    }
    for (size_t i = 0; i < taken.size(); i++) taken[i]->mTable.ready = true;
}

} // namespace orbx_adapter
