// adapter/pnp/PnPsolver.h -- drop-in for the reference's include/PnPsolver.h: the same public interface, the EPnP RANSAC hypotheses on
// the device.  The constructor does the reference's gather on the host (src/PnPsolver.cc:69-113).  The first iterate() or find() draws
// mRansacMaxIts sample rows and evaluates them in ONE call (orbx_pnp_hypotheses: compute_pose on the four, CheckInliers on every
// correspondence and, for a row that reaches mRansacMinInliers, Refine from the row's own inliers; one wave per hypothesis), and every call
// then replays the reference's loop (:176-269) over the table.  The loop condition of the reference is an OR, so a solver that is called
// again after mRansacMaxIts runs nIterations rows beyond it: those rows are drawn and evaluated by a second small call, only when the
// replay reaches them.
// orbx_adapter::PnPsolverBatch evaluates the tables of every candidate's solver of one Relocalization in one launch: one line after the
// loop that creates the solvers (src/Tracking.cc:1674-1700).
//
// STATED DEVIATIONS (include/orbx.h).  Every OpenCV call of EPnP (cvSVD, cvInvert, cvSolve) is restated as one Jacobi SVD, so
// results differ from the reference's at rounding level -- and, for a minimal set of four, by the basis of a null space.  qr_solve's x is
// defined as zero where the reference reads it uninitialised.  Refine reads the best ROW's own refinement from the table, which is what
// the reference computes (include/orbx.h).  The random stream: the reference draws four indices per iteration as it goes; a solver here
// draws mRansacMaxIts rows at its first iterate (or in PnPsolverBatch, solver by solver).  The draw is the same, the stream is not.
// Its own sub-directory, like adapter/sim3/: it needs Frame::mvLevelSigma2 and DUtils::Random.
#ifndef PNPSOLVER_H
#define PNPSOLVER_H

#include <stdint.h>
#include <vector>

#include <opencv2/core/core.hpp>
#include "MapPoint.h"
#include "Frame.h"

namespace ORB_SLAM2
{
class PnPsolver;
}

namespace orbx_adapter
{
// Evaluates every solver of the list that has no table yet (NULL entries and solvers with fewer correspondences than
// mRansacMinInliers are passed over) in ONE orbx_pnp_hypotheses_batch per 64 jobs.  Throws std::runtime_error when the library refuses.
void PnPsolverBatch(std::vector<ORB_SLAM2::PnPsolver *> &vpSolvers);
}

namespace ORB_SLAM2
{

class PnPsolver {
 public:
  PnPsolver(const Frame &F, const std::vector<MapPoint*> &vpMapPointMatches);

  ~PnPsolver();

  void SetRansacParameters(double probability = 0.99, int minInliers = 8 , int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                           float th2 = 5.991);

  cv::Mat find(std::vector<bool> &vbInliers, int &nInliers);

  cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

#ifdef ORBX_ADAPTER_CAPTURE
  // test hook (tests/adapter_pnp_driver.cc): what the solver hands to the ABI and what came back.  Not in a production build.
  struct Capture {
    int N, n_matches, min_inliers, max_its, rows;
    const double *K;
    const std::vector<float> *P3Dw, *P2D, *sigma2, *max_err;
    const std::vector<size_t> *indices;
    const std::vector<int32_t> *samples, *n_inliers, *n_refined;
    const std::vector<double> *Rt, *Rt_refined;
    const std::vector<uint64_t> *bits, *refined_bits;
  };
  Capture capture() const;
#endif

 private:
  friend void orbx_adapter::PnPsolverBatch(std::vector<PnPsolver *> &vpSolvers);

  // one row per hypothesis: what went to the call and what came back
  struct Table {
    int rows;                                        // evaluated so far
    std::vector<int32_t> samples, count, refined;    // [rows][4], [rows], [rows]
    std::vector<double> Rt, RtRefined;               // [rows][12]
    std::vector<uint64_t> bits, refinedBits;         // [rows][words]
    Table() : rows(0) {}
  };
  bool NeedsTable() const;            // enough correspondences to iterate at all, and no table yet
  void Draw(int rows);                // `rows` more sample rows through DUtils::Random::RandomInt, and room for their results
  void Evaluate(int rows);            // Draw + one call for them
  cv::Mat Pose(const double *Rt) const;
  void Scatter(const uint64_t *bits, std::vector<bool> &vbInliers) const;

  // one entry per correspondence, in the order of the gather
  std::vector<float> mvP3Dw, mvP2D;                  // [N][3], [N][2]
  std::vector<float> mvSigma2, mvMaxError;           // [N]
  std::vector<size_t> mvKeyPointIndices;
  size_t mnMatches;                                  // mvpMapPointMatches.size()
  double mK[4];                                      // fu fv uc vc
  int N;

  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts, mRansacMinSet;
  float mRansacEpsilon;

  Table mTable;
  int mnIterations, mnBestInliers;                   // they persist across iterate() calls
  // the best row so far, copied out of the table: mBestTcw / mvbBestInliers, and what Refine makes of them
  std::vector<double> mBestRt, mBestRefinedRt;       // [12]
  std::vector<uint64_t> mBestBits, mBestRefinedBits; // [words]
  int mnBestRefined;
};

} //namespace ORB_SLAM

#endif //PNPSOLVER_H
