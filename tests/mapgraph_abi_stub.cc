// A host stand-in for the orbx_mapgraph part of the ABI (include/orbx.h), on std::map and std::vector, for the stand-alone run of the adaptor's
// host bookkeeping (adapter/mapgraph/MapGraph.cc: slots, queue, echoes) under the address and undefined-behaviour sanitizers, where no GPU and no
// liborbx.so are involved (tests/test_mapgraph_adapter.py).  It refuses what the library refuses, so that a wrong slot or a batch with a key
// named twice fails the run.
#include <stdarg.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include <orbx.h>

static char g_err[256] = "";
static int refuse(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *orbx_last_error(void) { return g_err; }

struct StubKf { int n; std::vector<int32_t> match; std::vector<uint8_t> octave, stereo, close; StubKf() : n(-1) {} };
struct StubPt { std::map<int, int> obs; int n_obs; bool live, bad; StubPt() : n_obs(0), live(false), bad(false) {} };
struct orbx_mapgraph {
    std::vector<StubKf> kf; std::vector<StubPt> pt; int max_feat, max_obs;
    std::vector<int32_t> went_bad;
    bool kf_ok(int k) const { return k >= 0 && k < (int)kf.size() && kf[k].n >= 0; }
    void set_bad(int p)
    {
        StubPt &P = pt[p];
        P.live = P.bad = true;
        for (std::map<int, int>::iterator it = P.obs.begin(); it != P.obs.end(); ++it) kf[it->first].match[it->second] = -1;
        P.obs.clear();
        went_bad.push_back(p);
    }
    void erase_obs(int p, int k)
    {
        StubPt &P = pt[p];
        std::map<int, int>::iterator it = P.obs.find(k);
        if (it == P.obs.end()) return;
        P.n_obs -= kf[k].stereo[it->second] ? 2 : 1;
        P.obs.erase(it);
        if (P.n_obs <= 2) set_bad(p);
    }
    void erase_kf(int k)
    {
        for (int i = 0; i < kf[k].n; i++) if (kf[k].match[i] >= 0) erase_obs(kf[k].match[i], k);
        kf[k].n = -1;
    }
};

extern "C" int orbx_mapgraph_create(int, int max_keyframes, int max_features, int max_points, int max_obs, orbx_mapgraph **out)
{
    if (!out || max_keyframes < 1 || max_features < 1 || max_points < 1 || max_obs < 4 || max_obs > 256) return refuse(ORBX_E_INVALID, "create");
    orbx_mapgraph *g = new orbx_mapgraph();
    g->kf.resize(max_keyframes); g->pt.resize(max_points); g->max_feat = max_features; g->max_obs = max_obs;
    *out = g;
    return ORBX_OK;
}
extern "C" void orbx_mapgraph_destroy(orbx_mapgraph *g) { delete g; }
extern "C" int orbx_mapgraph_clear(orbx_mapgraph *g)
{
    std::fill(g->kf.begin(), g->kf.end(), StubKf()); std::fill(g->pt.begin(), g->pt.end(), StubPt());
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_set_keyframe(orbx_mapgraph *g, int kf, int n, const uint8_t *octave, const uint8_t *stereo, const uint8_t *close)
{
    if (kf < 0 || kf >= (int)g->kf.size() || n < 0 || n > g->max_feat || g->kf[kf].n >= 0) return refuse(ORBX_E_INVALID, "set_keyframe %d: n %d, in use %d", kf, n, kf >= 0 && kf < (int)g->kf.size() ? g->kf[kf].n : -2);
    if (orbx_mapgraph_keyframe_observations(g, kf) > 0) return refuse(ORBX_E_INVALID, "set_keyframe %d: observations still name the slot", kf);
    StubKf &K = g->kf[kf];
    K.n = n; K.match.assign(n, -1); K.octave.assign(octave, octave + n); K.stereo.assign(stereo, stereo + n); K.close.assign(close, close + n);
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_keyframe_observations(orbx_mapgraph *g, int kf)
{
    if (kf < 0 || kf >= (int)g->kf.size()) return refuse(ORBX_E_INVALID, "keyframe_observations: slot %d", kf);
    int n = 0;
    for (size_t p = 0; p < g->pt.size(); p++) n += (int)g->pt[p].obs.count(kf);
    return n;
}
extern "C" int orbx_mapgraph_set_matches(orbx_mapgraph *g, int kf, const int32_t *idx, const int32_t *point, int n)
{
    if (!g->kf_ok(kf)) return refuse(ORBX_E_INVALID, "set_matches: keyframe slot %d not in use", kf);
    std::set<int> seen;
    for (int i = 0; i < n; i++)
        if (idx[i] < 0 || idx[i] >= g->kf[kf].n || point[i] < -1 || point[i] >= (int)g->pt.size() || !seen.insert(idx[i]).second) return refuse(ORBX_E_INVALID, "set_matches: entry %d", i);
    for (int i = 0; i < n; i++) g->kf[kf].match[idx[i]] = point[i];
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_add_observations(orbx_mapgraph *g, const int32_t *point, const int32_t *kf, const int32_t *idx, int n)
{
    std::set<std::pair<int, int> > seen;
    for (int i = 0; i < n; i++)
        if (point[i] < 0 || point[i] >= (int)g->pt.size() || !g->kf_ok(kf[i]) || idx[i] < 0 || idx[i] >= g->kf[kf[i]].n || !seen.insert(std::make_pair(point[i], kf[i])).second)
            return refuse(ORBX_E_INVALID, "add_observations: entry %d (point %d, keyframe %d, feature %d)", i, point[i], kf[i], idx[i]);
    for (int i = 0; i < n; i++) {
        StubPt &P = g->pt[point[i]];
        if (P.bad) P = StubPt();
        if (P.obs.count(kf[i])) continue;
        if ((int)P.obs.size() == g->max_obs) return refuse(ORBX_E_CAPACITY, "add_observations: row of point %d full", point[i]);   // (no roll-back here: the run fails)
        P.obs[kf[i]] = idx[i];
        P.n_obs += g->kf[kf[i]].stereo[idx[i]] ? 2 : 1;
        P.live = true;
    }
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_erase_observations(orbx_mapgraph *g, const int32_t *point, const int32_t *kf, int n)
{
    std::set<std::pair<int, int> > seen;
    for (int i = 0; i < n; i++)
        if (point[i] < 0 || point[i] >= (int)g->pt.size() || kf[i] < 0 || kf[i] >= (int)g->kf.size() || !seen.insert(std::make_pair(point[i], kf[i])).second)
            return refuse(ORBX_E_INVALID, "erase_observations: entry %d", i);
    for (int i = 0; i < n; i++) g->erase_obs(point[i], kf[i]);
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_erase_points(orbx_mapgraph *g, const int32_t *point, int n)
{
    std::set<int> seen;
    for (int i = 0; i < n; i++)
        if (point[i] < 0 || point[i] >= (int)g->pt.size() || !seen.insert(point[i]).second) return refuse(ORBX_E_INVALID, "erase_points: entry %d", i);
    for (int i = 0; i < n; i++) g->set_bad(point[i]);
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_erase_keyframe(orbx_mapgraph *g, int kf)
{
    if (!g->kf_ok(kf)) return refuse(ORBX_E_INVALID, "erase_keyframe: keyframe slot %d not in use", kf);
    g->erase_kf(kf);
    return ORBX_OK;
}

static void count_rows(orbx_mapgraph *g, const int32_t *points, int n, int exclude, int32_t *counts, int32_t *nz, int *n_nz)
{
    std::fill(counts, counts + g->kf.size(), 0);
    for (int i = 0; i < n; i++) {
        if (points[i] < 0) continue;
        const StubPt &P = g->pt[points[i]];
        if (!P.live || P.bad) continue;
        for (std::map<int, int>::const_iterator it = P.obs.begin(); it != P.obs.end(); ++it) if (it->first != exclude) counts[it->first]++;
    }
    int m = 0;
    for (size_t k = 0; k < g->kf.size(); k++) if (counts[k]) { if (nz) nz[m] = (int32_t)k; m++; }
    if (n_nz) *n_nz = m;
}
extern "C" int orbx_mapgraph_vote(orbx_mapgraph *g, const int32_t *points, int n, int32_t *counts, int32_t *nz_slots, int *n_nz)
{
    for (int i = 0; i < n; i++) if (points[i] < 0 || points[i] >= (int)g->pt.size()) return refuse(ORBX_E_INVALID, "vote: entry %d", i);
    count_rows(g, points, n, -1, counts, nz_slots, n_nz);
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_covisibility(orbx_mapgraph *g, int kf, int32_t *counts, int32_t *nz_slots, int *n_nz)
{
    if (!g->kf_ok(kf)) return refuse(ORBX_E_INVALID, "covisibility: keyframe slot %d not in use", kf);
    count_rows(g, g->kf[kf].match.data(), g->kf[kf].n, kf, counts, nz_slots, n_nz);
    return ORBX_OK;
}
extern "C" int orbx_mapgraph_cull_keyframes(orbx_mapgraph *g, const int32_t *local, const uint8_t *not_erase, int n_local, int monocular,
                                            uint8_t *culled, int32_t *n_mps, int32_t *n_redundant, int32_t *bad_points, int cap, int *n_bad)
{
    std::set<int> seen;
    for (int j = 0; j < n_local; j++) if (!g->kf_ok(local[j]) || !seen.insert(local[j]).second) return refuse(ORBX_E_INVALID, "cull_keyframes: entry %d", j);
    g->went_bad.clear();
    for (int j = 0; j < n_local; j++) {
        const StubKf &K = g->kf[local[j]];
        int mps = 0, red = 0;
        for (int i = 0; i < K.n; i++) {
            if (K.match[i] < 0) continue;
            const StubPt &P = g->pt[K.match[i]];
            if (!P.live || P.bad || !(monocular || K.close[i])) continue;
            mps++;
            if (P.n_obs <= 3) continue;
            int others = 0;
            for (std::map<int, int>::const_iterator it = P.obs.begin(); it != P.obs.end(); ++it)
                if (it->first != local[j] && g->kf[it->first].octave[it->second] <= K.octave[i] + 1) others++;
            red += others >= 3;
        }
        if (n_mps) n_mps[j] = mps;
        if (n_redundant) n_redundant[j] = red;
        culled[j] = (double)red > 0.9 * (double)mps ? (not_erase[j] ? 2 : 1) : 0;
        if (culled[j] == 1) g->erase_kf(local[j]);
    }
    std::sort(g->went_bad.begin(), g->went_bad.end());
    *n_bad = (int)g->went_bad.size();
    if (*n_bad > cap) return refuse(ORBX_E_CAPACITY, "cull_keyframes: %d bad points, cap %d", *n_bad, cap);
    std::copy(g->went_bad.begin(), g->went_bad.end(), bad_points);
    return ORBX_OK;
}
