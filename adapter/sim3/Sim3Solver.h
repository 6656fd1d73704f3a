// adapter/sim3/Sim3Solver.h -- drop-in for the reference's include/Sim3Solver.h: the same public interface, the RANSAC hypotheses on
// the device.  The constructor does the reference's gather on the host (src/Sim3Solver.cc:37-113).  The first iterate() or find() draws
// ALL mRansacMaxIts sample triples, evaluates them in ONE call (orbx_sim3_hypotheses: Horn's closed form, both reprojections of every
// correspondence and the count, one wave per hypothesis), and every call then replays the reference's loop (:143-211) over the table:
// best-so-far on >=, return on > mRansacMinInliers, bNoMore after the loop.
// orbx_adapter::Sim3SolverBatch evaluates the tables of every solver of a ComputeSim3 call in one launch: one line after the loop that
// creates the solvers (src/LoopClosing.cc:293-340).
//
// STATED DEVIATIONS (include/orbx.h).  The rotation is evaluated algebraically from the quaternion instead of through atan2
// and cv::Rodrigues, and cv::eigen is restated as a cyclic Jacobi: results differ from the reference's at rounding level.  The random
// stream: the reference draws from one global rand() stream, five hypotheses per candidate in turn, and stops at a success; a solver
// here draws its whole sequence at its first iterate (or in Sim3SolverBatch, solver by solver).  The distribution is the same, the
// stream is not.  Given a solver's triple sequence, every iterate() result equals the reference algorithm as modelled.
// Its own sub-directory, like adapter/pose/ and adapter/triangulate/: it needs KeyFrame::mK and DUtils::Random.
#ifndef SIM3SOLVER_H
#define SIM3SOLVER_H

#include <stdint.h>
#include <vector>

#include <opencv2/opencv.hpp>

#include "KeyFrame.h"

namespace ORB_SLAM2
{
class Sim3Solver;
class MapPoint;
}

namespace orbx_adapter
{
// Evaluates every solver of the list that has no table yet (NULL entries and solvers with fewer correspondences than
// mRansacMinInliers are passed over) in ONE orbx_sim3_hypotheses_batch per 64 jobs.  Throws std::runtime_error when the library refuses.
void Sim3SolverBatch(std::vector<ORB_SLAM2::Sim3Solver *> &vpSolvers);
}

namespace ORB_SLAM2
{

class Sim3Solver
{
public:

    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*> &vpMatched12, const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6 , int maxIterations = 300);

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

#ifdef ORBX_ADAPTER_CAPTURE
    // test hook (tests/adapter_sim3_driver.cc): what the solver hands to the ABI and what came back.  Not in a production build.
    struct Capture {
        int N, mN1, max_its, fix_scale;
        const std::vector<float> *X1, *X2, *max_err1, *max_err2;
        const float *K1, *K2;
        const std::vector<size_t> *indices1;
        const std::vector<int32_t> *samples, *n_inliers;
        const std::vector<float> *srt;
        const std::vector<uint64_t> *bits;
    };
    Capture capture() const;
#endif

protected:
    friend void orbx_adapter::Sim3SolverBatch(std::vector<Sim3Solver *> &vpSolvers);

    // one row per hypothesis: what went to the call and what came back
    struct Table {
        bool ready;
        std::vector<int32_t> samples, count;       // [its][3], [its]
        std::vector<float> srt;                    // [its][13]
        std::vector<uint64_t> bits;                // [its][words]
        Table() : ready(false) {}
    };
    bool NeedsTable() const;           // enough correspondences to iterate at all, and no table yet
    void Draw();                       // mMaxIts triples through DUtils::Random::RandomInt, and room for their results
    cv::Mat Pose(const float *srt) const;

    // one entry per correspondence, in the order of the gather; mIndex1[i] = its index in vpMatched12 (the reference's mvnIndices1)
    std::vector<float> mX1, mX2;                   // [N][3] the points in camera 1 / camera 2 coordinates
    std::vector<float> mMaxErr1, mMaxErr2;         // [N] the truncated thresholds (include/orbx.h, "size_t")
    std::vector<size_t> mIndex1;
    float mK1[4], mK2[4];                          // fx fy cx cy
    int N, mN1;
    bool mbFixScale;

    double mProb;
    int mMinInliers, mMaxIts;

    Table mTable;
    int mnIterations, mnBestInliers;               // both persist across iterate() calls; SetRansacParameters resets the first only
    std::vector<float> mBest;                      // the best row's 13 floats (empty: none yet)
};

} //namespace ORB_SLAM

#endif // SIM3SOLVER_H
