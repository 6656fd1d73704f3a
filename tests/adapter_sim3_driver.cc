// tests/adapter_sim3_driver.cc -- ORB_SLAM2::Sim3Solver and orbx_adapter::Sim3SolverBatch (adapter/sim3/Sim3Solver.cc) on a stub map of one
// current keyframe and three loop candidates whose points are the current keyframe's under a drift similarity, with pixel-size noise and a
// share of wrong matches.  The match lists hold a null match, a bad point on either side, a point without an index in its keyframe on
// either side and a feature of the current keyframe without a point; the third candidate has fewer correspondences than minInliers.
// Built by tests/test_sim3_adapter.py with -DORBX_ADAPTER_CAPTURE against tests/cvstub_sim3 in front of tests/cvstub.
//   adapter_sim3_driver check
//   adapter_sim3_driver bench <candidates> <correspondences> <reps>     (tools/bench_sim3.py)
// checks the gather (indices, truncated thresholds, camera coordinates) against its own loop; that Sim3SolverBatch followed by rounds of
// iterate(5) gives, per candidate, the same returns as solvers evaluated one by one on the same random stream; and that both equal a
// replay, written here, over the table the ABI call returns for the captured inputs.  Prints "adaptor sim3 ok".
#include <math.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <vector>

#include <orbx.h>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Sim3Solver.h"
#include "orbx_device.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;
using ORB_SLAM2::Sim3Solver;

namespace {

int N1 = 160, NC = 200;            // features of the current keyframe / of a candidate (the bench mode sets them)
const int MIN_INLIERS = 20, ROUNDS = 12;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 12345) {}
    double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double uni(double a, double b) { return a + (b - a) * uni(); }
    double gauss() { return sqrt(-2.0 * log(uni() + 1e-300)) * cos(6.283185307179586 * uni()); }
};

cv::Mat mat3(const double R[9])
{
    cv::Mat m(3, 3, CV_32F);
    for (int k = 0; k < 9; k++) m.at<float>(k / 3, k % 3) = (float)R[k];
    return m;
}

cv::Mat vec3(double x, double y, double z)
{
    cv::Mat m(3, 1, CV_32F);
    m.at<float>(0) = (float)x; m.at<float>(1) = (float)y; m.at<float>(2) = (float)z;
    return m;
}

void rotation(double ax, double ay, double az, double ang, double R[9])
{
    const double n = sqrt(ax * ax + ay * ay + az * az), x = ax / n, y = ay / n, z = az / n, c = cos(ang), s = sin(ang), v = 1 - c;
    const double r[9] = { c + x * x * v, x * y * v - z * s, x * z * v + y * s, y * x * v + z * s, c + y * y * v, y * z * v - x * s,
                          z * x * v - y * s, z * y * v + x * s, c + z * z * v };
    memcpy(R, r, sizeof r);
}

void setup_keyframe(KeyFrame &kf, int n, const double R[9], double tx, double ty, double tz, const float K[4], Rng &rng)
{
    kf.N = n;
    kf.Rcw = mat3(R); kf.tcw = vec3(tx, ty, tz);
    kf.mK = cv::Mat(3, 3, CV_32F);
    for (int k = 0; k < 9; k++) kf.mK.at<float>(k / 3, k % 3) = 0.f;
    kf.mK.at<float>(0, 0) = K[0]; kf.mK.at<float>(1, 1) = K[1]; kf.mK.at<float>(0, 2) = K[2]; kf.mK.at<float>(1, 2) = K[3]; kf.mK.at<float>(2, 2) = 1.f;
    kf.mvScaleFactors.assign(8, 1.f); kf.mvLevelSigma2.assign(8, 1.f);
    for (int l = 1; l < 8; l++) kf.mvScaleFactors[l] = kf.mvScaleFactors[l - 1] * 1.2f;
    for (int l = 0; l < 8; l++) kf.mvLevelSigma2[l] = kf.mvScaleFactors[l] * kf.mvScaleFactors[l];
    kf.mvKeysUn.resize(n);
    for (int i = 0; i < n; i++) kf.mvKeysUn[i].octave = (int)(rng.uni() * 8) & 7;
    kf.mvpMapPoints.assign(n, (MapPoint *)NULL);
}

struct Result {
    bool empty, no_more; int n_inliers; std::vector<bool> inliers; std::vector<float> T;
    bool operator==(const Result &o) const
    {
        return empty == o.empty && no_more == o.no_more && n_inliers == o.n_inliers && inliers == o.inliers && T.size() == o.T.size() &&
               (T.empty() || memcmp(&T[0], &o.T[0], 4 * T.size()) == 0);
    }
};

Result round_of(Sim3Solver &s)
{
    Result r;
    const cv::Mat T = s.iterate(5, r.no_more, r.inliers, r.n_inliers);
    r.empty = T.empty();
    if (!r.empty)
        for (int k = 0; k < 16; k++) r.T.push_back(T.at<float>(k / 4, k % 4));
    return r;
}

int fail(const char *what, int a = -1, int b = -1)
{
    fprintf(stderr, "FAIL: %s (%d, %d)\n", what, a, b);
    return 1;
}

struct World {
    KeyFrame kf1;
    std::vector<KeyFrame> cand;
    std::vector<MapPoint> mp1;
    std::vector<std::vector<MapPoint> > mpc;
    std::vector<std::vector<MapPoint *> > matched;
    std::vector<bool> fix;
};

// special: the check mode's third candidate with four matches, and the cases the gather filters
void build(World &w, int ncand, bool special)
{
    w.cand.resize(ncand); w.mpc.resize(ncand); w.matched.resize(ncand); w.fix.resize(ncand);
    Rng rng(20);
    const float K1[4] = { 718.856f, 718.856f, 607.1928f, 185.2157f }, K2[4] = { 535.4f, 539.2f, 320.1f, 247.6f };
    double R[9];
    rotation(0.1, 1.0, 0.2, 0.15, R);
    setup_keyframe(w.kf1, N1, R, 0.2, -0.1, 0.5, K1, rng);
    w.mp1.assign(N1, MapPoint());
    std::vector<double> P(3 * N1);
    for (int i = 0; i < N1; i++) {
        P[3 * i] = rng.uni(-2.5, 2.5); P[3 * i + 1] = rng.uni(-1.5, 1.5); P[3 * i + 2] = rng.uni(4.0, 10.0);
        w.mp1[i].mWorldPos = vec3(P[3 * i], P[3 * i + 1], P[3 * i + 2]);
        w.mp1[i].AddObservation(&w.kf1, (size_t)i);
        w.kf1.mvpMapPoints[i] = &w.mp1[i];
    }
    for (int c = 0; c < ncand; c++) {
        double Rc[9], Rd[9];
        rotation(0.3, 1.0, -0.1 * (c % 3), 0.1 + 0.05 * (c % 3), Rc);
        setup_keyframe(w.cand[c], NC, Rc, -0.3 + 0.2 * (c % 3), 0.05, 0.8, c == 1 ? K1 : K2, rng);
        w.fix[c] = c == 1;
        const double sd = w.fix[c] ? 1.0 : 1.15 + 0.1 * (c % 3);            // the drift between the two visits of the place
        rotation(1.0, 0.2 * (c % 3), 0.4, 0.05 + 0.02 * (c % 3), Rd);
        w.mpc[c].assign(NC, MapPoint());
        w.matched[c].assign(N1, (MapPoint *)NULL);
        for (int i = 0; i < N1; i++) {
            if (special && c == 2 ? i % 40 != 1 : rng.uni() < 0.2) continue;      // candidate 2 keeps four matches
            const int j = (i * 7 + 3 * c) % NC;                        // its feature in the candidate
            const bool wrong = rng.uni() < 0.4;
            const double *p = &P[3 * (wrong ? (i + 17) % N1 : i)];
            double q[3];
            for (int r = 0; r < 3; r++) q[r] = sd * (Rd[3 * r] * p[0] + Rd[3 * r + 1] * p[1] + Rd[3 * r + 2] * p[2]) + 0.1 * (r + 1) + 0.02 * rng.gauss();
            w.mpc[c][j].mWorldPos = vec3(q[0], q[1], q[2]);
            w.mpc[c][j].AddObservation(&w.cand[c], (size_t)j);
            w.cand[c].mvpMapPoints[j] = &w.mpc[c][j];
            w.matched[c][i] = &w.mpc[c][j];
        }
    }
    if (!special) return;
    // the cases the gather filters: (the matches named here exist in candidates 0 and 1: set them first)
    for (int c = 0; c < 2; c++)
        for (int i = 3; i <= 13; i += 2)
            if (!w.matched[c][i]) {
                const int j = (i * 7 + 3 * c) % NC;
                w.mpc[c][j].mWorldPos = vec3(0.1 * i, 0.2, 6.0);
                w.mpc[c][j].AddObservation(&w.cand[c], (size_t)j);
                w.matched[c][i] = &w.mpc[c][j];
            }
    w.matched[0][3] = NULL; w.matched[1][3] = NULL;                   // a null match
    w.mp1[5].mbBad = true;                                            // a bad point of the current keyframe
    w.matched[1][7]->mbBad = true;                                    // a bad point of candidate 1
    w.mp1[9].mObservations.clear();                                   // a point without an index in the current keyframe
    w.matched[0][11]->mObservations.clear();                          // ... and in candidate 0
    w.kf1.mvpMapPoints[13] = NULL;                                    // a feature of the current keyframe without a point
}

// the gather of src/Sim3Solver.cc:62-104, written on its own
int check_gather(World &w, int c, const Sim3Solver::Capture &cap)
{
    std::vector<size_t> idx;
    std::vector<float> e1, e2, X1, X2;
    for (int i = 0; i < N1; i++) {
        MapPoint *m2 = w.matched[c][i], *m1 = w.kf1.mvpMapPoints[i];
        if (!m2 || !m1 || m1->mbBad || m2->mbBad) continue;
        if (!m1->mObservations.count(&w.kf1) || !m2->mObservations.count(&w.cand[c])) continue;
        const int o1 = w.kf1.mvKeysUn[m1->mObservations[&w.kf1]].octave, o2 = w.cand[c].mvKeysUn[m2->mObservations[&w.cand[c]]].octave;
        const double full1 = 9.210 * w.kf1.mvLevelSigma2[o1], full2 = 9.210 * w.cand[c].mvLevelSigma2[o2];
        e1.push_back((float)floor(full1)); e2.push_back((float)floor(full2));
        if ((double)e1.back() == full1) return fail("a threshold that truncation does not change", c, i);
        idx.push_back((size_t)i);
        const cv::Mat a = w.kf1.Rcw * m1->mWorldPos + w.kf1.tcw, b = w.cand[c].Rcw * m2->mWorldPos + w.cand[c].tcw;
        for (int r = 0; r < 3; r++) { X1.push_back(a.at<float>(r)); X2.push_back(b.at<float>(r)); }
    }
    if (cap.N != (int)idx.size() || cap.mN1 != N1) return fail("N", cap.N, (int)idx.size());
    if (*cap.indices1 != idx) return fail("mvnIndices1", c);
    if (*cap.max_err1 != e1 || *cap.max_err2 != e2) return fail("thresholds", c);
    if (*cap.X1 != X1 || *cap.X2 != X2) return fail("camera coordinates", c);
    for (size_t k = 0; k < idx.size(); k++)
        if (idx[k] == 3 || idx[k] == 5 || idx[k] == 9 || idx[k] == 13 || (c == 1 && idx[k] == 7) || (c == 0 && idx[k] == 11))
            return fail("a filtered match was gathered", c, (int)idx[k]);
    const cv::Mat &K = w.cand[c].mK;
    if (cap.K2[0] != K.at<float>(0, 0) || cap.K2[1] != K.at<float>(1, 1) || cap.K2[2] != K.at<float>(0, 2) || cap.K2[3] != K.at<float>(1, 2)) return fail("K2", c);
    return 0;
}

// iterate over a table, written on its own: rounds of five
std::vector<Result> replay(const Sim3Solver::Capture &cap, const std::vector<int32_t> &count, const std::vector<float> &srt, const std::vector<uint64_t> &bits)
{
    std::vector<Result> out;
    const size_t words = ((size_t)cap.N + 63) / 64;
    int it = 0, best = 0;
    for (int round = 0; round < ROUNDS; round++) {
        Result r;
        r.empty = true; r.no_more = false; r.n_inliers = 0; r.inliers.assign(N1, false);
        if (cap.N < MIN_INLIERS) { r.no_more = true; out.push_back(r); continue; }
        bool returned = false;
        for (int k = 0; k < 5 && it < cap.max_its && !returned; k++) {
            const int h = it++;
            if (count[h] >= best) {
                best = count[h];
                if (count[h] > MIN_INLIERS) {
                    returned = true; r.empty = false; r.n_inliers = count[h];
                    for (int i = 0; i < cap.N; i++)
                        if ((bits[words * h + (i >> 6)] >> (i & 63)) & 1) r.inliers[(*cap.indices1)[i]] = true;
                    const float *s = &srt[13 * (size_t)h];
                    for (int a = 0; a < 3; a++) {
                        for (int b = 0; b < 3; b++) r.T.push_back((float)((double)s[0] * (double)s[1 + 3 * a + b]));
                        r.T.push_back(s[10 + a]);
                    }
                    r.T.push_back(0.f); r.T.push_back(0.f); r.T.push_back(0.f); r.T.push_back(1.f);
                }
            }
        }
        if (!returned) r.no_more = it >= cap.max_its;
        out.push_back(r);
    }
    return out;
}

int check()
{
    World w;
    build(w, 3, true);
    // A: the batch, then rounds; B: one by one on the same stream (each solver draws its whole sequence at its first iterate)
    std::vector<Sim3Solver *> A, B;
    for (int c = 0; c < 3; c++) {
        A.push_back(new Sim3Solver(&w.kf1, &w.cand[c], w.matched[c], w.fix[c]));
        B.push_back(new Sim3Solver(&w.kf1, &w.cand[c], w.matched[c], w.fix[c]));
        A[c]->SetRansacParameters(0.99, MIN_INLIERS, 300);
        B[c]->SetRansacParameters(0.99, MIN_INLIERS, 300);
        if (int rc = check_gather(w, c, A[c]->capture())) return rc;
    }
    A.push_back(NULL);                                  // a discarded candidate's slot
    if (A[2]->capture().N != 4) return fail("candidate 2 should keep four correspondences", A[2]->capture().N);
    DUtils::Random::SeedRand(77);
    orbx_adapter::Sim3SolverBatch(A);
    if (!A[2]->capture().samples->empty()) return fail("a solver below minInliers was evaluated");
    DUtils::Random::SeedRand(77);                       // the draw of src/Sim3Solver.cc:166-181, literally: a fresh copy of the indices per hypothesis
    for (int c = 0; c < 2; c++) {
        const Sim3Solver::Capture cap = A[c]->capture();
        std::vector<int32_t> expect;
        for (int h = 0; h < cap.max_its; h++) {
            std::vector<size_t> avail;
            for (int i = 0; i < cap.N; i++) avail.push_back((size_t)i);
            for (int k = 0; k < 3; k++) {
                const int r = DUtils::Random::RandomInt(0, (int)avail.size() - 1);
                expect.push_back((int32_t)avail[r]);
                avail[r] = avail.back();
                avail.pop_back();
            }
        }
        if (*cap.samples != expect) return fail("the draw is not the reference's swap-remove procedure", c);
    }
    std::vector<std::vector<Result> > ra(3), rb(3);
    for (int round = 0; round < ROUNDS; round++)
        for (int c = 0; c < 3; c++) ra[c].push_back(round_of(*A[c]));
    DUtils::Random::SeedRand(77);
    for (int round = 0; round < ROUNDS; round++)
        for (int c = 0; c < 3; c++) rb[c].push_back(round_of(*B[c]));
    int returns = 0;
    for (int c = 0; c < 3; c++) {
        const Sim3Solver::Capture ca = A[c]->capture(), cb = B[c]->capture();
        if (*ca.samples != *cb.samples) return fail("the two forms drew different triples", c);
        if (*ca.n_inliers != *cb.n_inliers || *ca.bits != *cb.bits || ca.srt->size() != cb.srt->size() ||
            (!ca.srt->empty() && memcmp(&(*ca.srt)[0], &(*cb.srt)[0], 4 * ca.srt->size()))) return fail("batch and single tables differ", c);
        for (int round = 0; round < ROUNDS; round++)
            if (!(ra[c][round] == rb[c][round])) return fail("batch and single returns differ", c, round);
        std::vector<int32_t> count; std::vector<float> srt; std::vector<uint64_t> bits;
        if (ca.N >= MIN_INLIERS) {
            const size_t words = ((size_t)ca.N + 63) / 64;
            count.assign(ca.max_its, -1); srt.assign(13 * (size_t)ca.max_its, -1.f); bits.assign(words * ca.max_its, ~(uint64_t)0);
            orbx_sim3_job j;
            memset(&j, 0, sizeof j);
            j.n = ca.N; j.X1 = &(*ca.X1)[0]; j.X2 = &(*ca.X2)[0]; j.max_err1 = &(*ca.max_err1)[0]; j.max_err2 = &(*ca.max_err2)[0];
            memcpy(j.K1, ca.K1, sizeof j.K1); memcpy(j.K2, ca.K2, sizeof j.K2);
            j.fix_scale = ca.fix_scale; j.n_hyp = ca.max_its; j.samples = &(*ca.samples)[0];
            j.n_inliers = &count[0]; j.srt = &srt[0]; j.inlier_bits = &bits[0];
            if (orbx_sim3_hypotheses(orbx_adapter::Device(), &j) != ORBX_OK) { fprintf(stderr, "orbx_sim3_hypotheses: %s\n", orbx_last_error()); return 1; }
            if (count != *ca.n_inliers || bits != *ca.bits || memcmp(&srt[0], &(*ca.srt)[0], 4 * srt.size())) return fail("the ABI call on the captured inputs differs", c);
        }
        const std::vector<Result> exp = replay(ca, count, srt, bits);
        for (int round = 0; round < ROUNDS; round++) {
            if (!(ra[c][round] == exp[round])) return fail("the adaptor's returns differ from the replay of the ABI table", c, round);
            returns += !exp[round].empty;
        }
        printf("candidate %d: N = %d, %d iterations, returns in rounds:", c, ca.N, ca.max_its);
        for (int round = 0; round < ROUNDS; round++)
            if (!ra[c][round].empty) printf(" %d(%d)", round, ra[c][round].n_inliers);
        printf("%s\n", ra[c][ROUNDS - 1].no_more ? " ... bNoMore" : "");
    }
    if (returns < 2) return fail("the scene should let candidates 0 and 1 return", returns);
    if (!ra[2][0].no_more || !ra[2][0].empty) return fail("candidate 2 has fewer correspondences than minInliers");
    if (A[0]->GetEstimatedRotation().empty() || A[0]->GetEstimatedScale() <= 0.f) return fail("no best estimate");
    if (fabsf(A[1]->GetEstimatedScale() - 1.0f) != 0.f) return fail("fix_scale");
    // a later SetRansacParameters draws and evaluates again
    A[0]->SetRansacParameters(0.99, MIN_INLIERS, 40);
    const std::vector<int32_t> before = *A[0]->capture().samples;
    round_of(*A[0]);
    if (A[0]->capture().max_its != 40 || A[0]->capture().samples->size() != 120 || *A[0]->capture().samples == before) return fail("SetRansacParameters keeps the table");
    for (size_t i = 0; i < A.size(); i++) delete A[i];
    for (size_t i = 0; i < B.size(); i++) delete B[i];
    orbx_thread_release();
    printf("adaptor sim3 ok\n");
    return 0;
}

double now_us()
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}

double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

// ComputeSim3's solver part for `ncand` candidates of about 0.8 * n correspondences, `reps` times: the constructors (the gather),
// SetRansacParameters(0.99, 20, 300), Sim3SolverBatch (the draw and ONE device call) and rounds of iterate(5) per candidate until it
// returns or has no more.  Prints the medians of the three parts and of their sum, in microseconds.
int bench(int ncand, int n, int reps)
{
    N1 = n * 5 / 4; NC = N1 + 40;
    World w;
    build(w, ncand, false);
    DUtils::Random::SeedRand(5);
    std::vector<double> t_make, t_batch, t_iter, t_all;
    int corr = 0, hyp = 0, found = 0;
    for (int rep = -5; rep < reps; rep++) {
        const double t0 = now_us();
        std::vector<Sim3Solver *> S;
        for (int c = 0; c < ncand; c++) {
            S.push_back(new Sim3Solver(&w.kf1, &w.cand[c], w.matched[c], w.fix[c]));
            S[c]->SetRansacParameters(0.99, MIN_INLIERS, 300);
        }
        const double t1 = now_us();
        orbx_adapter::Sim3SolverBatch(S);
        const double t2 = now_us();
        corr = hyp = found = 0;
        for (int c = 0; c < ncand; c++) {
            bool more = false; std::vector<bool> in; int ni = 0;
            while (!more && S[c]->iterate(5, more, in, ni).empty()) {}
            found += ni > 0;
        }
        const double t3 = now_us();
        for (int c = 0; c < ncand; c++) { corr += S[c]->capture().N; hyp += S[c]->capture().max_its; delete S[c]; }
        if (rep < 0) continue;
        t_make.push_back(t1 - t0); t_batch.push_back(t2 - t1); t_iter.push_back(t3 - t2); t_all.push_back(t3 - t0);
    }
    printf("adaptor %d candidates x %d correspondences (%d in all), %d hypotheses, %d candidates found: gather %.1f  draw + device call %.1f  replay %.1f  "
           "all %.1f\n", ncand, corr / ncand, corr, hyp, found, median(t_make), median(t_batch), median(t_iter), median(t_all));
    orbx_thread_release();
    return 0;
}

}   // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 5 && !strcmp(argv[1], "bench")) return bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    fprintf(stderr, "usage: %s check | bench <candidates> <correspondences> <reps>\n", argv[0]);
    return 2;
}
