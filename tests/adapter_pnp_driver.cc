// tests/adapter_pnp_driver.cc -- ORB_SLAM2::PnPsolver and orbx_adapter::PnPsolverBatch (adapter/pnp/PnPsolver.cc) on a stub frame and three
// relocalisation candidates whose match lists pair the frame's keypoints with map points seen from a known pose, with pixel noise and a
// share of wrong matches.  The match lists hold null matches and bad points; the third candidate has fewer correspondences than
// mRansacMinInliers.  Built by tests/test_pnp_adapter.py with -DORBX_ADAPTER_CAPTURE against tests/cvstub_pnp in front of tests/cvstub.
//   adapter_pnp_driver check
//   adapter_pnp_driver bench <candidates> <correspondences> <reps>     (tools/bench_pnp.py)
// checks the gather (indices, sigma2, thresholds, points) against its own loop; the draw against the reference's swap-remove procedure;
// that PnPsolverBatch followed by rounds of iterate(5) gives, per candidate, the same returns as solvers evaluated one by one on the same
// random stream; and that both equal a replay, written here, over the table the ABI call returns for the captured inputs -- the rows past
// mRansacMaxIts included.  Prints "adaptor pnp ok".
#include <math.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <vector>

#include <orbx.h>

#include "Frame.h"
#include "MapPoint.h"
#include "PnPsolver.h"
#include "orbx_device.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"

using ORB_SLAM2::Frame;
using ORB_SLAM2::MapPoint;
using ORB_SLAM2::PnPsolver;

float Frame::fx = 718.856f, Frame::fy = 718.856f, Frame::cx = 607.1928f, Frame::cy = 185.2157f;

namespace {

int NF = 160;                      // keypoints of the frame (the bench mode sets it)
const int ROUNDS = 12;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 12345) {}
    double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double uni(double a, double b) { return a + (b - a) * uni(); }
    double gauss() { return sqrt(-2.0 * log(uni() + 1e-300)) * cos(6.283185307179586 * uni()); }
};

void rotation(double ax, double ay, double az, double ang, double R[9])
{
    const double n = sqrt(ax * ax + ay * ay + az * az), x = ax / n, y = ay / n, z = az / n, c = cos(ang), s = sin(ang), v = 1 - c;
    const double r[9] = { c + x * x * v, x * y * v - z * s, x * z * v + y * s, y * x * v + z * s, c + y * y * v, y * z * v - x * s,
                          z * x * v - y * s, z * y * v + x * s, c + z * z * v };
    memcpy(R, r, sizeof r);
}

struct Result {
    bool empty, no_more; int n_inliers; std::vector<bool> inliers; std::vector<float> T;
    bool operator==(const Result &o) const
    {
        return empty == o.empty && no_more == o.no_more && n_inliers == o.n_inliers && inliers == o.inliers && T.size() == o.T.size() &&
               (T.empty() || memcmp(&T[0], &o.T[0], 4 * T.size()) == 0);
    }
};

Result round_of(PnPsolver &s)
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
    Frame F;
    std::vector<std::vector<MapPoint> > mp;              // per candidate, one point per keypoint of the frame
    std::vector<std::vector<MapPoint *> > matched;
};

// special: the check mode's third candidate with six matches, and the cases the gather filters
void build(World &w, int ncand, bool special)
{
    Rng rng(31);
    w.F.N = NF;
    w.F.mvKeysUn.resize(NF);
    w.F.mvLevelSigma2.assign(8, 1.f);
    float sf = 1.f;
    for (int l = 0; l < 8; l++) { w.F.mvLevelSigma2[l] = sf * sf; sf *= 1.2f; }
    w.F.mvpMapPoints.assign(NF, (MapPoint *)NULL);
    double R[9];
    rotation(0.3, -0.8, 0.5, 0.35, R);
    const double t[3] = { 0.25, -0.15, 0.3 };
    std::vector<double> Xc(3 * (size_t)NF);
    for (int i = 0; i < NF; i++) {
        double *p = &Xc[3 * (size_t)i];
        p[0] = rng.uni(-2.5, 2.5); p[1] = rng.uni(-1.5, 1.5); p[2] = rng.uni(3.0, 9.0);
        cv::KeyPoint &kp = w.F.mvKeysUn[i];
        kp.pt.x = (float)(Frame::fx * p[0] / p[2] + Frame::cx + 0.5 * rng.gauss());
        kp.pt.y = (float)(Frame::fy * p[1] / p[2] + Frame::cy + 0.5 * rng.gauss());
        kp.octave = (int)(rng.uni() * 8) & 7;
    }
    w.mp.resize(ncand); w.matched.resize(ncand);
    for (int c = 0; c < ncand; c++) {
        w.mp[c].resize(NF);
        w.matched[c].assign(NF, (MapPoint *)NULL);
        for (int i = 0; i < NF; i++) {
            const bool wrong = rng.uni() < 0.3;
            double p[3] = { Xc[3 * (size_t)i], Xc[3 * (size_t)i + 1], Xc[3 * (size_t)i + 2] };
            if (wrong) { p[0] = rng.uni(-2.5, 2.5); p[1] = rng.uni(-1.5, 1.5); p[2] = rng.uni(3.0, 9.0); }
            cv::Mat pos(3, 1, CV_32F);                   // Xw = R^T (Xc - t)
            for (int r = 0; r < 3; r++)
                pos.at<float>(r) = (float)(R[r] * (p[0] - t[0]) + R[3 + r] * (p[1] - t[1]) + R[6 + r] * (p[2] - t[2]));
            w.mp[c][i].mWorldPos = pos;
            const bool keep = special && c == 2 ? i % 27 == 3 : rng.uni() < 0.8;      // SearchByBoW leaves many keypoints without a match
            if (keep) w.matched[c][i] = &w.mp[c][i];
        }
        if (special) {
            for (int i = 5; i < NF; i += 17) w.mp[c][i].mbBad = true;                  // a bad point is passed over (:87)
        }
    }
}

int check_gather(const World &w, int c, const PnPsolver::Capture &cap, float th2)
{
    std::vector<size_t> idx; std::vector<float> p3, p2, s2, me;
    for (int i = 0; i < NF; i++) {
        MapPoint *p = w.matched[c][i];
        if (!p || p->isBad()) continue;
        idx.push_back((size_t)i);
        p2.push_back(w.F.mvKeysUn[i].pt.x); p2.push_back(w.F.mvKeysUn[i].pt.y);
        s2.push_back(w.F.mvLevelSigma2[w.F.mvKeysUn[i].octave]);
        me.push_back(s2.back() * th2);
        for (int r = 0; r < 3; r++) p3.push_back(p->mWorldPos.at<float>(r));
    }
    if (cap.N != (int)idx.size() || cap.n_matches != NF) return fail("gather: N", c, cap.N);
    if (*cap.indices != idx || *cap.P3Dw != p3 || *cap.P2D != p2 || *cap.sigma2 != s2 || *cap.max_err != me) return fail("gather: arrays", c);
    if (cap.K[0] != (double)Frame::fx || cap.K[1] != (double)Frame::fy || cap.K[2] != (double)Frame::cx || cap.K[3] != (double)Frame::cy) return fail("gather: K", c);
    return 0;
}

struct Tab { std::vector<int32_t> count, refined; std::vector<double> Rt, RtR; std::vector<uint64_t> bits, rbits; };

void push_pose(Result &r, const double *Rt)
{
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) r.T.push_back((float)Rt[3 * a + b]);
        r.T.push_back((float)Rt[9 + a]);
    }
    r.T.push_back(0.f); r.T.push_back(0.f); r.T.push_back(0.f); r.T.push_back(1.f);
}

void scatter(Result &r, const PnPsolver::Capture &cap, const uint64_t *bits)
{
    r.inliers.assign(NF, false);
    for (int i = 0; i < cap.N; i++)
        if ((bits[i >> 6] >> (i & 63)) & 1) r.inliers[(*cap.indices)[i]] = true;
}

// iterate over a table, written on its own: rounds of five with the reference's OR condition; Refine reads the best row's refinement
std::vector<Result> replay(const PnPsolver::Capture &cap, const Tab &t)
{
    std::vector<Result> out;
    const size_t words = ((size_t)cap.N + 63) / 64;
    int it = 0, best = 0, best_row = -1;
    for (int round = 0; round < ROUNDS; round++) {
        Result r;
        r.empty = true; r.no_more = false; r.n_inliers = 0;
        if (cap.N < cap.min_inliers) { r.no_more = true; out.push_back(r); continue; }
        bool returned = false;
        for (int k = 0; (it < cap.max_its || k < 5) && !returned; k++) {
            const int h = it++;
            if (t.count[h] < cap.min_inliers) continue;
            if (t.count[h] > best) { best = t.count[h]; best_row = h; }
            if (t.refined[best_row] > cap.min_inliers) {
                returned = true; r.empty = false; r.n_inliers = t.refined[best_row];
                scatter(r, cap, &t.rbits[words * best_row]);
                push_pose(r, &t.RtR[12 * (size_t)best_row]);
            }
        }
        if (!returned && it >= cap.max_its) {
            r.no_more = true;
            if (best >= cap.min_inliers) {
                r.empty = false; r.n_inliers = best;
                scatter(r, cap, &t.bits[words * best_row]);
                push_pose(r, &t.Rt[12 * (size_t)best_row]);
            }
        }
        out.push_back(r);
    }
    return out;
}

int check()
{
    World w;
    build(w, 3, true);
    const float th2 = 5.991f;
    // A: the batch, then rounds; B: one by one on the same stream (a solver draws mRansacMaxIts rows at its first iterate)
    std::vector<PnPsolver *> A, B;
    for (int c = 0; c < 3; c++) {
        A.push_back(new PnPsolver(w.F, w.matched[c]));
        B.push_back(new PnPsolver(w.F, w.matched[c]));
        A[c]->SetRansacParameters(0.99, 10, 300, 4, 0.5, th2);      // Tracking::Relocalization's arguments
        B[c]->SetRansacParameters(0.99, 10, 300, 4, 0.5, th2);
        if (int rc = check_gather(w, c, A[c]->capture(), th2)) return rc;
    }
    A.push_back(NULL);                                  // a discarded candidate's slot
    if (A[0]->capture().max_its != 35 || A[0]->capture().min_inliers != A[0]->capture().N / 2) return fail("SetRansacParameters", A[0]->capture().max_its);
    if (A[2]->capture().N >= 10 || A[2]->capture().N < 4) return fail("candidate 2 should keep fewer than ten correspondences", A[2]->capture().N);
    DUtils::Random::SeedRand(77);
    orbx_adapter::PnPsolverBatch(A);
    if (!A[2]->capture().samples->empty()) return fail("a solver below mRansacMinInliers was evaluated");
    DUtils::Random::SeedRand(77);                       // the draw of src/PnPsolver.cc:199-212, literally: a fresh copy of the indices per row
    for (int c = 0; c < 2; c++) {
        const PnPsolver::Capture cap = A[c]->capture();
        std::vector<int32_t> expect;
        for (int h = 0; h < cap.max_its; h++) {
            std::vector<size_t> avail;
            for (int i = 0; i < cap.N; i++) avail.push_back((size_t)i);
            for (int k = 0; k < 4; k++) {
                const int r = DUtils::Random::RandomInt(0, (int)avail.size() - 1);
                expect.push_back((int32_t)avail[r]);
                avail[r] = avail.back();
                avail.pop_back();
            }
        }
        if (cap.rows != cap.max_its || *cap.samples != expect) return fail("the draw is not the reference's swap-remove procedure", c);
    }
    // (the streams of A and B now differ in position only by what the literal draw above consumed: both are re-seeded below)
    std::vector<std::vector<Result> > ra(3), rb(3);
    DUtils::Random::SeedRand(78);                       // the tails of A
    for (int round = 0; round < ROUNDS; round++)
        for (int c = 0; c < 3; c++) ra[c].push_back(round_of(*A[c]));
    DUtils::Random::SeedRand(77);
    for (int c = 0; c < 3; c++) rb[c].push_back(round_of(*B[c]));      // the tables of B, in the batch's order
    DUtils::Random::SeedRand(78);                       // the tails of B
    for (int round = 1; round < ROUNDS; round++)
        for (int c = 0; c < 3; c++) rb[c].push_back(round_of(*B[c]));
    int returns = 0, tails = 0;
    for (int c = 0; c < 3; c++) {
        const PnPsolver::Capture ca = A[c]->capture(), cb = B[c]->capture();
        if (*ca.samples != *cb.samples) return fail("the two forms drew different rows", c);
        if (*ca.n_inliers != *cb.n_inliers || *ca.bits != *cb.bits || *ca.n_refined != *cb.n_refined || *ca.refined_bits != *cb.refined_bits ||
            ca.Rt->size() != cb.Rt->size() || (!ca.Rt->empty() && (memcmp(&(*ca.Rt)[0], &(*cb.Rt)[0], 8 * ca.Rt->size()) ||
                                                                  memcmp(&(*ca.Rt_refined)[0], &(*cb.Rt_refined)[0], 8 * ca.Rt->size()))))
            return fail("batch and single tables differ", c);
        for (int round = 0; round < ROUNDS; round++)
            if (!(ra[c][round] == rb[c][round])) return fail("batch and single returns differ", c, round);
        Tab t;
        if (ca.N >= ca.min_inliers) {
            const size_t words = ((size_t)ca.N + 63) / 64, rows = (size_t)ca.rows;
            t.count.assign(rows, -7); t.refined.assign(rows, -7); t.Rt.assign(12 * rows, -1.0); t.RtR.assign(12 * rows, -1.0);
            t.bits.assign(words * rows, ~(uint64_t)0); t.rbits.assign(words * rows, ~(uint64_t)0);
            orbx_pnp_job j;
            memset(&j, 0, sizeof j);
            j.n = ca.N; j.P3Dw = &(*ca.P3Dw)[0]; j.P2D = &(*ca.P2D)[0]; j.max_err = &(*ca.max_err)[0];
            memcpy(j.K, ca.K, sizeof j.K);
            j.min_inliers = ca.min_inliers; j.n_hyp = ca.rows; j.samples = &(*ca.samples)[0];
            j.n_inliers = &t.count[0]; j.Rt = &t.Rt[0]; j.inlier_bits = &t.bits[0];
            j.n_refined = &t.refined[0]; j.Rt_refined = &t.RtR[0]; j.refined_bits = &t.rbits[0];
            if (orbx_pnp_hypotheses(orbx_adapter::Device(), &j) != ORBX_OK) { fprintf(stderr, "orbx_pnp_hypotheses: %s\n", orbx_last_error()); return 1; }
            if (t.count != *ca.n_inliers || t.bits != *ca.bits || t.refined != *ca.n_refined || t.rbits != *ca.refined_bits ||
                memcmp(&t.Rt[0], &(*ca.Rt)[0], 8 * t.Rt.size()) || memcmp(&t.RtR[0], &(*ca.Rt_refined)[0], 8 * t.RtR.size()))
                return fail("the ABI call on the captured inputs differs", c);
            tails += ca.rows > ca.max_its;
        }
        const std::vector<Result> exp = replay(ca, t);
        for (int round = 0; round < ROUNDS; round++) {
            if (!(ra[c][round] == exp[round])) return fail("the adaptor's returns differ from the replay of the ABI table", c, round);
            returns += !exp[round].empty && !exp[round].no_more;
        }
        printf("candidate %d: N = %d, min inliers %d, %d iterations, %d rows evaluated, returns in rounds:", c, ca.N, ca.min_inliers, ca.max_its, ca.rows);
        for (int round = 0; round < ROUNDS; round++)
            if (!ra[c][round].empty) printf(" %d(%d)", round, ra[c][round].n_inliers);
        printf("\n");
    }
    if (returns < 2) return fail("the scene should let candidates 0 and 1 return a refined pose", returns);
    if (tails < 1) return fail("no solver was called again past mRansacMaxIts", tails);
    if (!ra[2][0].no_more || !ra[2][0].empty) return fail("candidate 2 has fewer correspondences than mRansacMinInliers");
    // a later SetRansacParameters draws and evaluates again
    A[0]->SetRansacParameters(0.99, 10, 20, 4, 0.5, th2);
    const std::vector<int32_t> before = *A[0]->capture().samples;
    if (!before.empty() || A[0]->capture().max_its != 20) return fail("SetRansacParameters keeps the table");
    for (size_t i = 0; i < A.size(); i++) delete A[i];
    for (size_t i = 0; i < B.size(); i++) delete B[i];
    orbx_thread_release();
    printf("adaptor pnp ok\n");
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

// Relocalization's solver part for `ncand` candidates of about 0.8 * n matches, `reps` times: the constructors (the gather),
// SetRansacParameters(0.99, 10, max_its, 4, 0.5, 5.991), PnPsolverBatch (the draw and ONE device call) and one iterate(5) per candidate.
// Prints the medians of the three parts and of their sum, in microseconds.
int bench(int ncand, int n, int max_its, int reps)
{
    NF = n * 5 / 4;
    World w;
    build(w, ncand, false);
    DUtils::Random::SeedRand(5);
    std::vector<double> t_make, t_batch, t_iter, t_all;
    int corr = 0, hyp = 0, found = 0;
    for (int rep = -5; rep < reps; rep++) {
        const double t0 = now_us();
        std::vector<PnPsolver *> S;
        for (int c = 0; c < ncand; c++) {
            S.push_back(new PnPsolver(w.F, w.matched[c]));
            // epsilon 0.5 gives 35 rows; a small epsilon lets max_its decide (the 300-row shape of tools/bench_pnp.py)
            S[c]->SetRansacParameters(0.99, 10, max_its, 4, max_its > 35 ? 0.1f : 0.5f, 5.991f);
        }
        const double t1 = now_us();
        orbx_adapter::PnPsolverBatch(S);
        const double t2 = now_us();
        corr = hyp = found = 0;
        for (int c = 0; c < ncand; c++) {
            bool more = false; std::vector<bool> in; int ni = 0;
            found += !S[c]->iterate(5, more, in, ni).empty();
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
    if (argc == 6 && !strcmp(argv[1], "bench")) return bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    fprintf(stderr, "usage: %s check | bench <candidates> <correspondences> <max iterations> <reps>\n", argv[0]);
    return 2;
}
