// One host core on the same map as tools/bench_mapgraph.py: the three walks of the observation graph and a keyframe's edits as plain C++
// loops over std::map<int, int> per map point, timed like the device calls (median of `reps`).  A LOWER BOUND for the reference's cost, not
// the reference: no mutexes, no std::map copies per point (GetObservations returns one by value), ints for pointers, nothing else running.
//   mapgraph_host_loop scene.bin reps      (scene.bin: int32 words written by tools/bench_mapgraph.py)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <map>
#include <vector>

struct Kf { std::vector<int> match; std::vector<uint8_t> octave, stereo, close; bool bad; };
struct Pt { std::map<int, int> obs; int n_obs; bool bad; };
static std::vector<Kf> kfs;
static std::vector<Pt> pts;

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> &v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static void add_obs(int p, int k, int i) { if (pts[p].obs.count(k)) return; pts[p].obs[k] = i; pts[p].n_obs += kfs[k].stereo[i] ? 2 : 1; }
static void set_bad(int p)
{
    pts[p].bad = true;
    std::map<int, int> obs;
    obs.swap(pts[p].obs);
    for (std::map<int, int>::iterator it = obs.begin(); it != obs.end(); ++it) kfs[it->first].match[it->second] = -1;
}
static void erase_obs(int p, int k)
{
    std::map<int, int>::iterator it = pts[p].obs.find(k);
    if (it == pts[p].obs.end()) return;
    pts[p].n_obs -= kfs[k].stereo[it->second] ? 2 : 1;
    pts[p].obs.erase(it);
    if (pts[p].n_obs <= 2) set_bad(p);
}
static void erase_kf(int k)
{
    for (size_t i = 0; i < kfs[k].match.size(); i++) if (kfs[k].match[i] >= 0) erase_obs(kfs[k].match[i], k);
    kfs[k].bad = true;
}

static int vote(const std::vector<int> &list, std::map<int, int> &counter)
{
    counter.clear();
    for (size_t i = 0; i < list.size(); i++) {
        if (list[i] < 0 || pts[list[i]].bad) continue;
        const std::map<int, int> &obs = pts[list[i]].obs;
        for (std::map<int, int>::const_iterator it = obs.begin(); it != obs.end(); ++it) counter[it->first]++;
    }
    return (int)counter.size();
}

static int cull(const std::vector<int> &local, bool mono)
{
    int culled = 0;
    for (size_t j = 0; j < local.size(); j++) {
        const Kf &K = kfs[local[j]];
        int n_points = 0, n_redundant = 0;
        for (size_t i = 0; i < K.match.size(); i++) {
            if (K.match[i] < 0 || pts[K.match[i]].bad || !(mono || K.close[i])) continue;
            n_points++;
            const Pt &P = pts[K.match[i]];
            if (P.n_obs <= 3) continue;
            int others = 0;
            for (std::map<int, int>::const_iterator it = P.obs.begin(); it != P.obs.end() && others < 3; ++it)
                if (it->first != local[j] && kfs[it->first].octave[it->second] <= K.octave[i] + 1) others++;
            n_redundant += others >= 3;
        }
        if (n_redundant > 0.9 * n_points) { erase_kf(local[j]); culled++; }
    }
    return culled;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin reps\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<int32_t> w;
    int32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    const int reps = atoi(argv[2]);
    size_t at = 0;
    const int n_kf = w[at++], n_feat = w[at++], n_pt = w[at++];
    kfs.resize(n_kf); pts.resize(n_pt);
    for (int k = 0; k < n_kf; k++) {
        Kf &K = kfs[k];
        K.bad = false; K.match.assign(n_feat, -1); K.octave.resize(n_feat); K.stereo.resize(n_feat); K.close.resize(n_feat);
        for (int i = 0; i < n_feat; i++) { const int a = w[at++]; K.octave[i] = a & 31; K.stereo[i] = (a >> 6) & 1; K.close[i] = (a >> 7) & 1; }
    }
    for (int p = 0; p < n_pt; p++) { pts[p].n_obs = 0; pts[p].bad = false; }
    const int n_obs = w[at++];
    const size_t obs_at = at;
    for (int e = 0; e < n_obs; e++) { const int p = w[at++], k = w[at++], i = w[at++]; kfs[k].match[i] = p; add_obs(p, k, i); }
    std::vector<double> t((size_t)reps);
    std::map<int, int> counter;
    int sink = 0;
    const int n_lists = w[at++];
    for (int l = 0; l < n_lists; l++) {
        const int kind = w[at++], n = w[at++];      // 0 vote list, 1 covisibility keyframe, 2 cull list, 3 a keyframe whose edits are timed
        std::vector<int> list(w.begin() + at, w.begin() + at + n);
        at += n;
        if (kind == 0) {
            for (int r = 0; r < reps; r++) { const double t0 = now_us(); sink += vote(list, counter); t[r] = now_us() - t0; }
            printf("host vote %d points: %.1f us (%d keyframes voted for)\n", n, median(t), (int)counter.size());
        } else if (kind == 1) {
            for (int r = 0; r < reps; r++) { const double t0 = now_us(); sink += vote(kfs[list[0]].match, counter); counter.erase(list[0]); t[r] = now_us() - t0; }
            printf("host covisibility keyframe %d: %.1f us (%d keyframes)\n", list[0], median(t), (int)counter.size());
        } else if (kind == 2) {
            int culled = 0;
            for (int r = 0; r < reps; r++) {
                const double t0 = now_us();
                culled = cull(list, true);
                t[r] = now_us() - t0;
                for (size_t j = 0; j < list.size(); j++) {          // outside the clock: the culled keyframes' observations back
                    if (!kfs[list[j]].bad) continue;
                    kfs[list[j]].bad = false;
                    for (int i = 0; i < n_feat; i++) if (kfs[list[j]].match[i] >= 0) add_obs(kfs[list[j]].match[i], list[j], i);
                }
            }
            printf("host cull %d local keyframes, %d culled: %.1f us\n", n, culled, median(t));
        } else {
            const int k = list[0];
            std::vector<int> match(kfs[k].match);
            for (int r = 0; r < reps; r++) {
                erase_kf(k);                                        // outside the clock
                std::fill(kfs[k].match.begin(), kfs[k].match.end(), -1);
                const double t0 = now_us();
                kfs[k].bad = false;
                for (int i = 0; i < n_feat; i++) if (match[i] >= 0) { kfs[k].match[i] = match[i]; add_obs(match[i], k, i); }
                t[r] = now_us() - t0;
            }
            printf("host edits of keyframe %d (%d matches and observations): %.1f us\n", k, (int)(n_feat - std::count(match.begin(), match.end(), -1)), median(t));
        }
    }
    (void)obs_at;
    return sink == -1;
}
