// adapter/init/Initializer.h -- drop-in for the reference's include/Initializer.h: the same public interface, Initialize on the device.
// The constructor keeps the reference frame's keypoints and mK (src/Initializer.cc:37-46).  Initialize gathers the keypoints of both
// frames, builds mvMatches12, draws mvSets with DUtils::Random exactly as :79-111 does (the reference itself draws all of them up front,
// so the random stream is the reference's) and hands everything to ONE call, orbx_mono_init_initialize: the H / F table, the choice, the
// decomposition, CheckRT of every motion hypothesis and the decision run as three launches on one stream, and only the result comes
// down.  Tracking::MonocularInitialization is unchanged.
//
// STATED DEVIATIONS (include/orbx.h).  Every cv::SVDecomp, inv and determinant of the file is restated, so results differ
// from the reference's at rounding level, and which of R1 / R2 comes first and the sign of t follow from the restated SVD (the set of
// motion hypotheses is the same).  A score is each lane's serial sum closed by a butterfly, not one serial sum.  When no hypothesis of
// the model taken scores above 0 the call returns false (the reference reads an empty matrix).  On false the outputs are left as they
// were (the reference clears R21 / t21 in ReconstructF only).  Fewer than eight matches return false without a call (the reference
// draws from an empty list); more than 8192 matches, or a refusal of the library, throw std::runtime_error.
// Its own sub-directory, like adapter/pnp/: it needs Frame::mK and DUtils::Random.
#ifndef INITIALIZER_H
#define INITIALIZER_H

#include <stdint.h>
#include <vector>

#include <opencv2/opencv.hpp>
#include "Frame.h"

namespace ORB_SLAM2
{

class Initializer
{
public:
    // the reference frame: its undistorted keypoints and mK are kept
    Initializer(const Frame &ReferenceFrame, float sigma = 1.0, int iterations = 200);

    // vMatches12[i] = the keypoint of CurrentFrame matched to keypoint i of the reference frame, or -1.  True: R21 (3 x 3), t21 (3 x 1),
    // vP3D and vbTriangulated (one entry per keypoint of the reference frame) hold the reconstruction.
    bool Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12,
                    cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated);

#ifdef ORBX_ADAPTER_CAPTURE
    // test hook (tests/adapter_init_driver.cc): what the last Initialize handed to the ABI and what came back.  Not in a production build.
    struct Capture {
        const std::vector<float> *xy1, *xy2, *P3D;
        const std::vector<int32_t> *matches, *samples;
        const std::vector<uint8_t> *triangulated;
        const std::vector<std::vector<size_t> > *sets;
        float K[4], sigma;
        int ok, model, best_h, best_f, winner;
        float R21[9], t21[3], parallax;
    };
    Capture capture() const;
#endif

private:
    std::vector<float> mXY1;                      // [n1][2] the reference frame's mvKeysUn[i].pt, gathered once
    float mK[4];                                  // fx fy cx cy of the reference frame's mK
    float mSigma;
    int mMaxIterations;
    std::vector<std::vector<size_t> > mvSets;     // the sample rows of the last Initialize, as the reference keeps them

    // what went to the last call and what came back
    std::vector<float> mXY2, mP3D;
    std::vector<int32_t> mMatches, mSamples;      // [n][2] mvMatches12, [iterations][8]
    std::vector<uint8_t> mTriangulated;
    int mLast[5];            // ok, model, best_h, best_f, winner
    float mLastRt[13];       // R21, t21, parallax
};

} //namespace ORB_SLAM

#endif // INITIALIZER_H
