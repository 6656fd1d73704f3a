// One host core on the same map as tools/bench_refresh.py: MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors as
// plain C++ loops over a std::map<int, int> per map point, timed like the device calls (median of `reps`).  A LOWER BOUND for the
// reference's cost, not the reference: no mutexes, no copy of the std::map per call, no cv::Mat per observer, no row clone per descriptor,
// ints for pointers, nothing else running.
//   refresh_host_loop scene.bin reps      (scene.bin: written by tools/bench_refresh.py)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <map>
#include <vector>

static int nkf, nfeat, npt, nobs, nlevels;
static std::vector<float> centre, pos, sf;
static std::vector<uint8_t> octave, desc;
static std::vector<int32_t> ref;
static std::vector<std::map<int, int> > rows;
static std::vector<float> out_geom;
static std::vector<uint8_t> out_desc;

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> &v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static void update_normal_and_depth(int p)
{
    const std::map<int, int> &obs = rows[p];
    if (obs.empty()) return;
    const float *P = &pos[3 * (size_t)p];
    float n[3] = { 0.f, 0.f, 0.f };
    for (std::map<int, int>::const_iterator it = obs.begin(); it != obs.end(); ++it) {
        const float *O = &centre[3 * (size_t)it->first];
        const float d[3] = { P[0] - O[0], P[1] - O[1], P[2] - O[2] };
        const double inv = 1.0 / sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
        for (int c = 0; c < 3; c++) n[c] = n[c] + (float)((double)d[c] * inv);
    }
    const int r = ref[p];
    std::map<int, int>::const_iterator it = obs.find(r);
    const int idx = it == obs.end() ? 0 : it->second;
    const float *O = &centre[3 * (size_t)r];
    const float d[3] = { P[0] - O[0], P[1] - O[1], P[2] - O[2] };
    const float dist = (float)sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
    float *g = &out_geom[8 * (size_t)p];
    g[7] = dist * sf[octave[(size_t)r * nfeat + idx]];
    g[3] = g[7] / sf[nlevels - 1];
    const double invn = 1.0 / (double)obs.size();
    for (int c = 0; c < 3; c++) { g[c] = P[c]; g[4 + c] = (float)((double)n[c] * invn); }
}

static int distance(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int w = 0; w < 4; w++) { uint64_t x, y; memcpy(&x, a + 8 * w, 8); memcpy(&y, b + 8 * w, 8); d += __builtin_popcountll(x ^ y); }
    return d;
}

static void distinctive(int p)
{
    const std::map<int, int> &obs = rows[p];
    if (obs.empty()) return;
    std::vector<const uint8_t *> v;
    v.reserve(obs.size());
    for (std::map<int, int>::const_iterator it = obs.begin(); it != obs.end(); ++it) v.push_back(&desc[32 * ((size_t)it->first * nfeat + it->second)]);
    const size_t N = v.size();
    std::vector<int> D(N * N, 0), row(N);
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) D[i * N + j] = D[j * N + i] = distance(v[i], v[j]);
    int best = 0x7FFFFFFF, bi = 0;
    for (size_t i = 0; i < N; i++) {
        std::copy(D.begin() + i * N, D.begin() + (i + 1) * N, row.begin());
        std::sort(row.begin(), row.end());
        const int m = row[(size_t)(0.5 * (N - 1))];
        if (m < best) { best = m; bi = (int)i; }
    }
    memcpy(&out_desc[32 * (size_t)p], v[bi], 32);
}

template <class T> static void rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); if (fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short scene\n"); exit(1); } }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: refresh_host_loop scene.bin reps\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    const int reps = atoi(argv[2]);
    std::vector<int32_t> head, obs;
    rd(f, head, 5);
    nkf = head[0]; nfeat = head[1]; npt = head[2]; nobs = head[3]; nlevels = head[4];
    rd(f, sf, (size_t)nlevels); rd(f, centre, 3 * (size_t)nkf); rd(f, octave, (size_t)nkf * nfeat); rd(f, desc, 32 * (size_t)nkf * nfeat);
    rd(f, pos, 3 * (size_t)npt); rd(f, ref, (size_t)npt); rd(f, obs, 3 * (size_t)nobs);
    fclose(f);
    rows.resize((size_t)npt);
    for (int i = 0; i < nobs; i++) rows[obs[3 * i]][obs[3 * i + 1]] = obs[3 * i + 2];
    out_geom.assign(8 * (size_t)npt, 0.f); out_desc.assign(32 * (size_t)npt, 0);
    const int sizes[3] = { 2000, 8000, npt };
    for (int s = 0; s < 3; s++) {
        const int n = std::min(sizes[s], npt);
        for (int what = 1; what <= 3; what++) {
            if (s == 2 && what != 1) continue;
            std::vector<double> t;
            for (int r = 0; r < reps; r++) {
                const double t0 = now_us();
                for (int p = 0; p < n; p++) { if (what & 1) update_normal_and_depth(p); if (what & 2) distinctive(p); }
                t.push_back(now_us() - t0);
            }
            printf("host %s, %d points: %.1f us\n", what == 1 ? "GEOM" : what == 2 ? "DESC" : "GEOM+DESC", n, median(t));
        }
    }
    double sum = 0;
    for (size_t i = 0; i < out_geom.size(); i++) sum += out_geom[i] == out_geom[i] ? out_geom[i] : 0;
    printf("checksum %.3f %d\n", sum, (int)out_desc[32]);
    return 0;
}
