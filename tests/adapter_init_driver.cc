// tests/adapter_init_driver.cc -- ORB_SLAM2::Initializer (adapter/init/Initializer.cc) on two stub frames that see a depth-varied cloud
// under a sideways translation (exact projections rounded to float), the matches scattered among unmatched keypoints and vMatches12
// holding -1 for those, then on a third frame that differs from the first by a pure rotation.  Built by tests/test_init_adapter.py with
// -DORBX_ADAPTER_CAPTURE against tests/cvstub_init in front of tests/cvstub.
//   adapter_init_driver check
//   adapter_init_driver bench <matches> <reps>     (tools/bench_init.py)
// checks the gather (keypoints, mvMatches12) against its own loop; mvSets against its own draw by the reference's swap-remove procedure
// on the same random stream -- the second Initialize continues the stream, SeedRandOnce seeds once; and every output against a replay
// of orbx_mono_init_initialize, written here, on the inputs the adaptor captured.  Prints "adaptor init ok".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <vector>

#include <orbx.h>

#include "Frame.h"
#include "Initializer.h"
#include "orbx_device.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"

using ORB_SLAM2::Frame;
using ORB_SLAM2::Initializer;

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 12345) {}
    double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double uni(double a, double b) { return a + (b - a) * uni(); }
};

const float FX = 500.f, FY = 500.f, CX = 320.f, CY = 240.f;

// two frames of n1 / n2 keypoints, the first n of them (shuffled into place by `first` / `second`) projections of one cloud; R about the
// y axis by `ang`, translation t
struct Scene {
    Frame f1, f2;
    std::vector<int> vMatches12;
    std::vector<int> first, second;
};

Scene make_scene(int n, uint64_t seed, double ang, const double t[3])
{
    Scene S;
    Rng rng(seed);
    const int n1 = n + n / 5 + 3, n2 = n + n / 7 + 5;
    S.f1.mK = cv::Mat(3, 3, CV_32F); S.f2.mK = cv::Mat(3, 3, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) S.f1.mK.at<float>(r, c) = S.f2.mK.at<float>(r, c) = 0.f;
    Frame *fs[2] = { &S.f1, &S.f2 };
    for (int k = 0; k < 2; k++) {
        cv::Mat &K = fs[k]->mK;
        K.at<float>(0, 0) = FX; K.at<float>(1, 1) = FY; K.at<float>(0, 2) = CX; K.at<float>(1, 2) = CY; K.at<float>(2, 2) = 1.f;
    }
    S.f1.mvKeysUn.resize(n1); S.f2.mvKeysUn.resize(n2);
    for (int i = 0; i < n1; i++) S.f1.mvKeysUn[i].pt = cv::Point2f((float)rng.uni(0, 640), (float)rng.uni(0, 480));
    for (int i = 0; i < n2; i++) S.f2.mvKeysUn[i].pt = cv::Point2f((float)rng.uni(0, 640), (float)rng.uni(0, 480));
    // every (n1 / n)-th slot of frame 1, a stride through frame 2
    S.vMatches12.assign(n1, -1);
    const double c = cos(ang), s = sin(ang);
    for (int i = 0; i < n; i++) {
        const int a = (int)((long long)i * n1 / n), b = (int)(((long long)i * 7919) % n2);
        if (std::find(S.second.begin(), S.second.end(), b) != S.second.end()) continue;
        const double X = rng.uni(-2.5, 2.5), Y = rng.uni(-1.8, 1.8), Z = rng.uni(4.0, 10.0);
        const double X2 = c * X + s * Z + t[0], Y2 = Y + t[1], Z2 = -s * X + c * Z + t[2];
        S.f1.mvKeysUn[a].pt = cv::Point2f((float)(FX * X / Z + CX), (float)(FY * Y / Z + CY));
        S.f2.mvKeysUn[b].pt = cv::Point2f((float)(FX * X2 / Z2 + CX), (float)(FY * Y2 / Z2 + CY));
        S.vMatches12[a] = b;
        S.first.push_back(a); S.second.push_back(b);
    }
    return S;
}

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

// :93-111 on the stream as it stands
std::vector<std::vector<size_t> > draw(int N, int iterations)
{
    std::vector<std::vector<size_t> > sets(iterations, std::vector<size_t>(8, 0));
    for (int it = 0; it < iterations; it++) {
        std::vector<size_t> avail(N);
        for (int i = 0; i < N; i++) avail[i] = i;
        for (size_t j = 0; j < 8; j++) {
            const int randi = DUtils::Random::RandomInt(0, avail.size() - 1);
            sets[it][j] = avail[randi];
            avail[randi] = avail.back();
            avail.pop_back();
        }
    }
    return sets;
}

// the adaptor's outputs of one Initialize against its capture, the driver's own gather and a replay of the ABI call
int compare(const Scene &S, const Initializer &ini, bool ok, const cv::Mat &R21, const cv::Mat &t21, const std::vector<cv::Point3f> &vP3D,
            const std::vector<bool> &vbTri, const std::vector<std::vector<size_t> > &sets)
{
    const Initializer::Capture c = ini.capture();
    const size_t n1 = S.f1.mvKeysUn.size(), n2 = S.f2.mvKeysUn.size(), n = S.first.size();
    CHECK(c.xy1->size() == 2 * n1 && c.xy2->size() == 2 * n2 && c.matches->size() == 2 * n, "sizes of the gather");
    for (size_t i = 0; i < n1; i++) CHECK((*c.xy1)[2 * i] == S.f1.mvKeysUn[i].pt.x && (*c.xy1)[2 * i + 1] == S.f1.mvKeysUn[i].pt.y, "xy1[%zu]", i);
    for (size_t i = 0; i < n2; i++) CHECK((*c.xy2)[2 * i] == S.f2.mvKeysUn[i].pt.x && (*c.xy2)[2 * i + 1] == S.f2.mvKeysUn[i].pt.y, "xy2[%zu]", i);
    for (size_t i = 0; i < n; i++) CHECK((*c.matches)[2 * i] == S.first[i] && (*c.matches)[2 * i + 1] == S.second[i], "match %zu", i);
    CHECK(*c.sets == sets, "mvSets is not the driver's draw on the same stream");
    for (size_t h = 0; h < sets.size(); h++)
        for (int j = 0; j < 8; j++) CHECK((*c.samples)[8 * h + j] == (int32_t)sets[h][j], "samples[%zu][%d]", h, j);
    CHECK(c.K[0] == FX && c.K[1] == FY && c.K[2] == CX && c.K[3] == CY && c.sigma == 1.0f, "K, sigma");

    // the replay: the ABI call on what the adaptor captured
    std::vector<float> P3D(3 * n1, -1.f);
    std::vector<uint8_t> tri(n1, 7);
    orbx_mono_init_job job;
    memset(&job, 0, sizeof job);
    job.n1 = (int)n1; job.n2 = (int)n2; job.xy1 = c.xy1->data(); job.xy2 = c.xy2->data(); job.n = (int)n; job.matches = c.matches->data();
    job.sigma = c.sigma; memcpy(job.K, c.K, sizeof job.K); job.min_parallax = 1.0f; job.min_triangulated = 50;
    job.n_hyp = (int)sets.size(); job.samples = c.samples->data();
    orbx_mono_init_result res;
    memset(&res, 0, sizeof res);
    res.P3D = P3D.data(); res.triangulated = tri.data();
    CHECK(orbx_mono_init_initialize(orbx_adapter::Device(), &job, &res) == ORBX_OK, "%s", orbx_last_error());
    CHECK(ok == (res.ok != 0) && c.ok == res.ok && c.model == res.model && c.best_h == res.best_h && c.best_f == res.best_f &&
          c.winner == res.winner, "ok / model / winners: %d %d %d %d %d", res.ok, res.model, res.best_h, res.best_f, res.winner);
    CHECK(!memcmp(c.R21, res.R21, sizeof res.R21) && !memcmp(c.t21, res.t21, sizeof res.t21) && !memcmp(&c.parallax, &res.parallax, 4), "R21, t21");
    CHECK(*c.P3D == P3D && *c.triangulated == tri, "P3D, triangulated");
    if (ok) {
        CHECK(R21.rows == 3 && R21.cols == 3 && t21.rows == 3 && t21.cols == 1, "shapes of R21, t21");
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) CHECK(R21.at<float>(r, k) == res.R21[3 * r + k], "R21(%d, %d)", r, k);
            CHECK(t21.at<float>(r) == res.t21[r], "t21(%d)", r);
        }
        CHECK(vP3D.size() == n1 && vbTri.size() == n1, "sizes of vP3D, vbTriangulated");
        for (size_t i = 0; i < n1; i++)
            CHECK(vP3D[i].x == P3D[3 * i] && vP3D[i].y == P3D[3 * i + 1] && vP3D[i].z == P3D[3 * i + 2] && vbTri[i] == (tri[i] != 0), "point %zu", i);
    }
    return 0;
}

int check()
{
    const double t[3] = { 0.6, 0.05, 0.03 }, t0[3] = { 0, 0, 0 };
    Scene S = make_scene(240, 5, 0.05, t);
    const int N = (int)S.first.size();
    CHECK(N > 200 && N < (int)S.f1.mvKeysUn.size(), "scene");
    Initializer ini(S.f1, 1.0, 200);
    cv::Mat R21, t21;
    std::vector<cv::Point3f> vP3D;
    std::vector<bool> vbTri;
    const bool ok = ini.Initialize(S.f2, S.vMatches12, R21, t21, vP3D, vbTri);      // SeedRandOnce(0) seeds here
    DUtils::Random::SeedRand(0);
    std::vector<std::vector<size_t> > sets = draw(N, 200);
    if (compare(S, ini, ok, R21, t21, vP3D, vbTri, sets)) return 1;
    CHECK(ok, "a noise-free cloud under a sideways translation initialises");
    const int model = ini.capture().model;
    int ntri = 0;
    for (size_t i = 0; i < vbTri.size(); i++) {
        ntri += vbTri[i];
        CHECK(!vbTri[i] || S.vMatches12[i] >= 0, "an unmatched keypoint is triangulated");
    }
    CHECK(ntri > 0.9 * N, "%d of %d matches triangulated", ntri, N);
    // the rotation is the scene's: about y by 0.05
    CHECK(fabs(R21.at<float>(0, 2) - sin(0.05)) < 1e-3 && fabs(R21.at<float>(1, 1) - 1.0) < 1e-3, "R21 is not the scene's rotation");
    CHECK(fabs(fabs(t21.at<float>(0)) - 0.6 / sqrt(0.36 + 0.0025 + 0.0009)) < 1e-2, "t21 is not the scene's direction");

    // a second call on the same object: the stream goes on (no new seed), a pure rotation does not initialise, the outputs stay
    Scene S2 = make_scene(240, 5, 0.05, t0);
    S2.f1 = S.f1;
    const cv::Mat Rkeep = R21.clone();
    const bool ok2 = ini.Initialize(S2.f2, S2.vMatches12, R21, t21, vP3D, vbTri);
    DUtils::Random::SeedRand(0);     // the stream is the process's: the driver repeats it from the seed, rows 0-199 then 200-399
    draw(N, 200);
    sets = draw(N, 200);
    if (compare(S2, ini, ok2, R21, t21, vP3D, vbTri, sets)) return 1;
    CHECK(!ok2, "a pure rotation must not initialise");
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) CHECK(R21.at<float>(r, k) == Rkeep.at<float>(r, k), "R21 changed on false");

    // fewer than eight matches: false, no call
    std::vector<int> few(S.vMatches12.size(), -1);
    for (int i = 0; i < 7; i++) few[S.first[i]] = S.second[i];
    CHECK(!ini.Initialize(S.f2, few, R21, t21, vP3D, vbTri), "seven matches");
    printf("adaptor init ok: %d matches, %d triangulated, model %d\n", N, ntri, model);
    return 0;
}

double now_us()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

int bench(int n, int reps)
{
    const double t[3] = { 0.6, 0.05, 0.03 };
    Scene S = make_scene(n, 9, 0.05, t);
    cv::Mat R21, t21;
    std::vector<cv::Point3f> vP3D;
    std::vector<bool> vbTri;
    std::vector<double> us;
    bool ok = false;
    for (int r = 0; r < reps + 5; r++) {
        const double a = now_us();
        Initializer ini(S.f1, 1.0, 200);
        ok = ini.Initialize(S.f2, S.vMatches12, R21, t21, vP3D, vbTri);
        if (r >= 5) us.push_back(now_us() - a);
    }
    std::sort(us.begin(), us.end());
    printf("adaptor %zu matches of %zu / %zu keypoints, 200 hypotheses, initialised %d: constructor + Initialize %.1f\n", S.first.size(),
           S.f1.mvKeysUn.size(), S.f2.mvKeysUn.size(), (int)ok, us[us.size() / 2]);
    return 0;
}

}   // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 4 && !strcmp(argv[1], "bench")) return bench(atoi(argv[2]), atoi(argv[3]));
    fprintf(stderr, "usage: %s check | bench <matches> <reps>\n", argv[0]);
    return 2;
}
