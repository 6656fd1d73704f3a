// adapter/pnp/PnPsolver.cc -- ORB_SLAM2::PnPsolver with the hypotheses on the device (adapter/pnp/PnPsolver.h): the gather of the
// reference's constructor (src/PnPsolver.cc:69-113), SetRansacParameters (:128-165), the draw of the sample rows (:199-212), ONE
// orbx_pnp_hypotheses(_batch) call, and the state machine of PnPsolver::iterate (:176-269) replayed over the table the call returns.
#include "PnPsolver.h"

#include <algorithm>
#include <limits.h>
#include <math.h>
#include <stdexcept>
#include <string>
#include <string.h>

#include <orbx.h>

#include "orbx_device.h"

#include "Thirdparty/DBoW2/DUtils/Random.h"

namespace ORB_SLAM2
{

PnPsolver::PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches)
    : mnMatches(vpMapPointMatches.size()), N(0), mnIterations(0), mnBestInliers(0), mnBestRefined(-1)
{
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        const cv::KeyPoint &kp = F.mvKeysUn[i];
        mvP2D.push_back(kp.pt.x); mvP2D.push_back(kp.pt.y);
        mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
        const cv::Mat Pos = pMP->GetWorldPos();
        for (int r = 0; r < 3; r++) mvP3Dw.push_back(Pos.at<float>(r));
        mvKeyPointIndices.push_back(i);
    }
    mK[0] = F.fx; mK[1] = F.fy; mK[2] = F.cx; mK[3] = F.cy;     // the reference's double members fu, fv, uc, vc
    SetRansacParameters();
}

PnPsolver::~PnPsolver() {}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)
{
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    mRansacEpsilon = epsilon;
    mRansacMinSet = minSet;
    N = (int)mvSigma2.size();

    int nMinInliers = N * mRansacEpsilon;
    if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;

    int nIterations = 1;
    if (mRansacMinInliers != N) {
        const double x = ceil(log(1 - mRansacProb) / log(1 - pow(mRansacEpsilon, 3)));
        // fewer correspondences than mRansacMinInliers: the logarithm is NaN and iterate() never loops
        nIterations = x == x ? (int)std::max((double)INT_MIN, std::min((double)INT_MAX, x)) : INT_MIN;
    }
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));

    mvMaxError.resize(mvSigma2.size());
    for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
    mTable = Table();     // other thresholds, another count: rows are drawn and evaluated again
}

bool PnPsolver::NeedsTable() const { return mTable.rows == 0 && N >= mRansacMinInliers && N >= 4 && mRansacMinSet == 4; }

void PnPsolver::Draw(int rows)
{
    const size_t have = (size_t)mTable.rows, all = have + (size_t)rows, words = ((size_t)N + 63) / 64;
    mTable.samples.resize(4 * all);
    // every row draws from the full list 0 .. N-1, the drawn index replaced by the last one that is left (:199-212).  The reference
    // copies the list per row; undoing the four replacements gives the same list without the copy.
    std::vector<int32_t> left((size_t)N);
    for (int i = 0; i < N; i++) left[i] = i;
    for (size_t h = have; h < all; h++) {
        int at[4];
        int32_t drawn[4], last[4];
        for (int k = 0; k < 4; k++) {
            at[k] = DUtils::Random::RandomInt(0, (int)left.size() - 1);
            drawn[k] = left[at[k]]; last[k] = left.back();
            mTable.samples[4 * h + k] = drawn[k];
            left[at[k]] = last[k];
            left.pop_back();
        }
        for (int k = 3; k >= 0; k--) { left.push_back(last[k]); left[at[k]] = drawn[k]; }
    }
    mTable.count.resize(all, 0); mTable.refined.resize(all, -1);
    mTable.Rt.resize(12 * all, 0.0); mTable.RtRefined.resize(12 * all, 0.0);
    mTable.bits.resize(words * all, 0); mTable.refinedBits.resize(words * all, 0);
}

// the job of rows first .. first + n_hyp - 1 of a solver's table (drawn, with room for their results)
static orbx_pnp_job job_of(int N, const std::vector<float> &P3Dw, const std::vector<float> &P2D, const std::vector<float> &maxErr, const double K[4],
                           int minInliers, int first, int n_hyp, std::vector<int32_t> &samples, std::vector<int32_t> &count, std::vector<double> &Rt,
                           std::vector<uint64_t> &bits, std::vector<int32_t> &refined, std::vector<double> &RtRefined, std::vector<uint64_t> &refinedBits)
{
    const size_t words = ((size_t)N + 63) / 64, f = (size_t)first;
    orbx_pnp_job j;
    memset(&j, 0, sizeof j);
    j.n = N;
    j.P3Dw = &P3Dw[0]; j.P2D = &P2D[0]; j.max_err = &maxErr[0];
    memcpy(j.K, K, sizeof j.K);
    j.min_inliers = minInliers;
    j.n_hyp = n_hyp;
    j.samples = &samples[4 * f];
    j.n_inliers = &count[f]; j.Rt = &Rt[12 * f]; j.inlier_bits = &bits[words * f];
    j.n_refined = &refined[f]; j.Rt_refined = &RtRefined[12 * f]; j.refined_bits = &refinedBits[words * f];
    return j;
}

void PnPsolver::Evaluate(int rows)
{
    const int first = mTable.rows;
    Draw(rows);
    for (int at = 0; at < rows; at += 1024) {     // a call takes 1024 hypotheses per job
        orbx_pnp_job j = job_of(N, mvP3Dw, mvP2D, mvMaxError, mK, mRansacMinInliers, first + at, std::min(1024, rows - at), mTable.samples,
                                mTable.count, mTable.Rt, mTable.bits, mTable.refined, mTable.RtRefined, mTable.refinedBits);
        if (orbx_pnp_hypotheses(orbx_adapter::Device(), &j) != ORBX_OK) throw std::runtime_error(std::string("PnPsolver: ") + orbx_last_error());
    }
    mTable.rows = first + rows;
}

cv::Mat PnPsolver::Pose(const double *Rt) const
{
    cv::Mat T(4, 4, CV_32F);     // eye, with Rcw and tcw converted CV_64F -> CV_32F (:228-234)
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T.at<float>(r, c) = (float)Rt[3 * r + c];
        T.at<float>(r, 3) = (float)Rt[9 + r];
        T.at<float>(3, r) = 0.f;
    }
    T.at<float>(3, 3) = 1.f;
    return T;
}

void PnPsolver::Scatter(const uint64_t *bits, std::vector<bool> &vbInliers) const
{
    vbInliers = std::vector<bool>(mnMatches, false);
    for (int i = 0; i < N; i++)
        if ((bits[i >> 6] >> (i & 63)) & 1) vbInliers[mvKeyPointIndices[i]] = true;
}

cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    if (mRansacMinSet != 4 || N < 4) throw std::runtime_error("PnPsolver: the device table is built for the minimal set of four");
    if (mTable.rows == 0) Evaluate(mRansacMaxIts);
    const size_t words = ((size_t)N + 63) / 64;
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {     // an OR, as in the reference
        nCurrentIterations++;
        const size_t h = (size_t)mnIterations++;
        if ((int)h >= mTable.rows) Evaluate(std::max((int)h + 1 - mTable.rows, std::max(1, nIterations)));     // the tail, when it is reached
        const int count = mTable.count[h];
        if (count < mRansacMinInliers) continue;
        if (count > mnBestInliers) {
            mnBestInliers = count;
            mBestRt.assign(&mTable.Rt[12 * h], &mTable.Rt[12 * h] + 12);
            mBestBits.assign(&mTable.bits[words * h], &mTable.bits[words * h] + words);
            // Refine reads mvbBestInliers: this row's own refinement is what it computes until a better row comes
            mnBestRefined = mTable.refined[h];
            mBestRefinedRt.assign(&mTable.RtRefined[12 * h], &mTable.RtRefined[12 * h] + 12);
            mBestRefinedBits.assign(&mTable.refinedBits[words * h], &mTable.refinedBits[words * h] + words);
        }
        if (mnBestRefined > mRansacMinInliers) {
            nInliers = mnBestRefined;
            Scatter(&mBestRefinedBits[0], vbInliers);
            return Pose(&mBestRefinedRt[0]);
        }
    }
    if (mnIterations >= mRansacMaxIts) {
        bNoMore = true;
        if (mnBestInliers >= mRansacMinInliers) {
            nInliers = mnBestInliers;
            Scatter(&mBestBits[0], vbInliers);
            return Pose(&mBestRt[0]);
        }
    }
    return cv::Mat();
}

cv::Mat PnPsolver::find(std::vector<bool> &vbInliers, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

#ifdef ORBX_ADAPTER_CAPTURE
PnPsolver::Capture PnPsolver::capture() const
{
    Capture c;
    c.N = N; c.n_matches = (int)mnMatches; c.min_inliers = mRansacMinInliers; c.max_its = mRansacMaxIts; c.rows = mTable.rows;
    c.K = mK;
    c.P3Dw = &mvP3Dw; c.P2D = &mvP2D; c.sigma2 = &mvSigma2; c.max_err = &mvMaxError;
    c.indices = &mvKeyPointIndices;
    c.samples = &mTable.samples; c.n_inliers = &mTable.count; c.n_refined = &mTable.refined;
    c.Rt = &mTable.Rt; c.Rt_refined = &mTable.RtRefined;
    c.bits = &mTable.bits; c.refined_bits = &mTable.refinedBits;
    return c;
}
#endif

} // namespace ORB_SLAM2

namespace orbx_adapter
{

void PnPsolverBatch(std::vector<ORB_SLAM2::PnPsolver *> &vpSolvers)
{
    std::vector<orbx_pnp_job> jobs;
    std::vector<ORB_SLAM2::PnPsolver *> taken;
    for (size_t i = 0; i < vpSolvers.size(); i++) {
        ORB_SLAM2::PnPsolver *p = vpSolvers[i];
        if (!p || !p->NeedsTable() || std::find(taken.begin(), taken.end(), p) != taken.end()) continue;
        taken.push_back(p);
        p->Draw(p->mRansacMaxIts);
        for (int first = 0; first < p->mRansacMaxIts; first += 1024)     // a call takes 1024 hypotheses per job
            jobs.push_back(ORB_SLAM2::job_of(p->N, p->mvP3Dw, p->mvP2D, p->mvMaxError, p->mK, p->mRansacMinInliers, first,
                                             std::min(1024, p->mRansacMaxIts - first), p->mTable.samples, p->mTable.count, p->mTable.Rt,
                                             p->mTable.bits, p->mTable.refined, p->mTable.RtRefined, p->mTable.refinedBits));
    }
    for (size_t at = 0; at < jobs.size(); at += 64) {                     // ... and 64 jobs
        const int nj = (int)std::min((size_t)64, jobs.size() - at);
        const int rc = nj == 1 ? orbx_pnp_hypotheses(Device(), &jobs[at]) : orbx_pnp_hypotheses_batch(Device(), &jobs[at], nj);
        if (rc != ORBX_OK) throw std::runtime_error(std::string("PnPsolver: ") + orbx_last_error());
    }
    for (size_t i = 0; i < taken.size(); i++) taken[i]->mTable.rows = taken[i]->mRansacMaxIts;
}

} // namespace orbx_adapter
