// Driver of adapter/mapgraph/MapGraph.cc (tests/test_mapgraph_adapter.py): builds a stub map twice through the stand-in mutators of
// tests/cvstub_graph -- once with the hooks firing, for the adaptor, once without, for plain host loops -- and compares the two maps
// object by object after LocalMapping::KeyFrameCulling, after more edits and a second culling, and the two vote functions in between.
//   adapter_mapgraph_driver check [mono]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <map>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Map.h"
#include "Frame.h"
#include "LocalMapping.h"
#include "MapGraph.h"

namespace ORB_SLAM2 { bool g_hooks = false; }
using namespace ORB_SLAM2;
using std::map;
using std::vector;

static unsigned g_rng;
static unsigned rnd(unsigned n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }

struct World {
    vector<void *> kf_mem, pt_mem;          // every object is built in storage of the world's own, so that an address can be used twice
    vector<KeyFrame *> kf;
    vector<MapPoint *> pt;
    long unsigned next_kf_id, next_pt_id;
    World() : next_kf_id(0), next_pt_id(0) {}
    int index(KeyFrame *p) const { for (size_t i = 0; i < kf.size(); i++) if (kf[i] == p) return (int)i; return -1; }
    int index(MapPoint *p) const { for (size_t i = 0; i < pt.size(); i++) if (pt[i] == p) return (int)i; return -1; }
    KeyFrame *new_kf(size_t slot, int n, bool stereo)
    {
        vector<int> oct(n); vector<float> ur(n), depth(n);
        for (int i = 0; i < n; i++) {
            oct[i] = rnd(16) == 0 ? 3 : 1 + (int)rnd(2);
            const bool st = stereo && rnd(10) < 7;
            ur[i] = st ? 10.f + (float)rnd(600) : -1.f;
            depth[i] = st ? (rnd(10) < 8 ? 1.f + (float)rnd(30) : 60.f) : -1.f;
        }
        if (kf_mem.size() <= slot) kf_mem.resize(slot + 1, (void *)NULL);
        if (!kf_mem[slot]) kf_mem[slot] = malloc(sizeof(KeyFrame));
        return new (kf_mem[slot]) KeyFrame(next_kf_id++, oct, ur, depth, 40.f);
    }
    MapPoint *new_pt(size_t slot)
    {
        if (pt_mem.size() <= slot) pt_mem.resize(slot + 1, (void *)NULL);
        if (!pt_mem[slot]) pt_mem[slot] = malloc(sizeof(MapPoint));
        return new (pt_mem[slot]) MapPoint(next_pt_id++);
    }
    void destroy()
    {
        for (size_t i = 0; i < kf.size(); i++) kf[i]->~KeyFrame();
        for (size_t i = 0; i < pt.size(); i++) pt[i]->~MapPoint();
        kf.clear(); pt.clear();
    }
    ~World()
    {
        destroy();
        for (size_t i = 0; i < kf_mem.size(); i++) free(kf_mem[i]);
        for (size_t i = 0; i < pt_mem.size(); i++) free(pt_mem[i]);
    }
};

static const int NK = 14, NF = 48, NP = 110;

// keyframe k observes point p at a free feature: both views, or (rarely) one of them
static void observe(World &w, vector<vector<int> > &free_feat, int k, int p, int how)
{
    if (free_feat[k].empty()) return;
    const int i = free_feat[k].back();
    free_feat[k].pop_back();
    if (how != 2) w.kf[k]->AddMapPoint(w.pt[p], i);
    if (how != 1) w.pt[p]->AddObservation(w.kf[k], i);
}

static void build(World &w, bool hooks, bool stereo, bool with_ghosts)
{
    g_hooks = hooks;
    if (with_ghosts) {
        // a first map, whose objects go away without a word to anybody (Map::clear deletes without SetBadFlag): the second map's
        // first keyframes and points are then made at the same addresses
        g_rng = 99;
        w.next_kf_id = 50;
        for (int k = 0; k < 3; k++) w.kf.push_back(w.new_kf(k, 20, stereo));
        for (int p = 0; p < 5; p++) {
            w.pt.push_back(w.new_pt(p));
            for (int k = 0; k < 3; k++) { w.kf[k]->AddMapPoint(w.pt[p], p); w.pt[p]->AddObservation(w.kf[k], p); }
        }
        orbx_adapter::MapGraph::instance().Flush();
        w.destroy();
    } else {
        w.next_kf_id = 3; w.next_pt_id = 5;
    }
    g_rng = 1234;
    w.next_kf_id = 0;                       // the map's first keyframe has mnId 0
    for (int k = 0; k < NK; k++) w.kf.push_back(w.new_kf(k, NF - (int)rnd(8), stereo));
    w.next_kf_id = 100;
    for (int p = 0; p < NP; p++) w.pt.push_back(w.new_pt(p));
    vector<vector<int> > free_feat(NK);
    for (int k = 0; k < NK; k++) for (int i = w.kf[k]->N - 1; i >= 0; i--) free_feat[k].push_back(i);
    for (int p = 0; p < NP; p++) {
        const int c = (int)rnd(NK), m = rnd(25) == 0 ? 2 : 4 + (int)rnd(3);
        for (int t = 0, seen = 0; t < 9 && seen < m; t++) {
            const int k = c - 4 + t;
            if (k < 0 || k >= NK || rnd(6) == 0) continue;
            const unsigned u = rnd(100);
            observe(w, free_feat, k, p, seen == 0 || u < 94 ? 0 : u < 97 ? 1 : 2);
            seen++;
        }
    }
    for (int p = 0; p < 4; p++) { w.pt[p]->AddObservation(w.kf[5], 0); w.pt[p]->AddObservation(w.kf[5], 1); }     // the second is a repeat: src/MapPoint.cc:109
    w.kf[4]->SetNotErase();
    KeyFrame *cur = w.kf[NK - 1];
    for (int k = 0; k < NK - 1; k++) cur->mvpOrderedConnectedKeyFrames.push_back(w.kf[(k * 5 + 3) % (NK - 1)]);     // keyframe 0 (mnId 0) among them
    g_hooks = false;
}

// ---- plain host loops on the stand-ins: what the three functions of the reference compute, written for this test

static void host_culling(KeyFrame *cur, bool mono)
{
    const vector<KeyFrame *> local = cur->GetVectorCovisibleKeyFrames();
    for (size_t j = 0; j < local.size(); j++) {
        KeyFrame *kf = local[j];
        if (kf->mnId == 0) continue;
        const vector<MapPoint *> pts = kf->GetMapPointMatches();
        int n_points = 0, n_redundant = 0;
        for (size_t i = 0; i < pts.size(); i++) {
            MapPoint *mp = pts[i];
            if (!mp || mp->isBad()) continue;
            if (!mono && (kf->mvDepth[i] > kf->mThDepth || kf->mvDepth[i] < 0)) continue;
            n_points++;
            if (mp->Observations() <= 3) continue;
            const map<KeyFrame *, size_t> obs = mp->GetObservations();
            int others = 0;
            for (map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it)
                if (it->first != kf && it->first->mvKeysUn[it->second].octave <= kf->mvKeysUn[i].octave + 1) others++;
            if (others >= 3) n_redundant++;
        }
        if (n_redundant > 0.9 * n_points) kf->SetBadFlag();
    }
}

static void host_covisibility(KeyFrame *kf, map<KeyFrame *, int> &counter)
{
    counter.clear();
    const vector<MapPoint *> pts = kf->GetMapPointMatches();
    for (size_t i = 0; i < pts.size(); i++) {
        if (!pts[i] || pts[i]->isBad()) continue;
        const map<KeyFrame *, size_t> obs = pts[i]->GetObservations();
        for (map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it)
            if (it->first->mnId != kf->mnId) counter[it->first]++;
    }
}

static void host_vote(Frame &F, map<KeyFrame *, int> &counter)
{
    counter.clear();
    for (int i = 0; i < F.N; i++) {
        MapPoint *mp = F.mvpMapPoints[i];
        if (!mp) continue;
        if (mp->isBad()) { F.mvpMapPoints[i] = NULL; continue; }
        const map<KeyFrame *, size_t> obs = mp->GetObservations();
        for (map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) counter[it->first]++;
    }
}

// ---- comparison, object by object through the indices

static int g_fail = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { printf("MISMATCH " __VA_ARGS__); printf("\n"); } } } while (0)

static void same_maps(const World &a, const World &b, const char *tag)
{
    EXPECT(a.kf.size() == b.kf.size() && a.pt.size() == b.pt.size(), "%s: sizes", tag);
    for (size_t k = 0; k < a.kf.size() && k < b.kf.size(); k++) {
        EXPECT(a.kf[k]->isBad() == b.kf[k]->isBad(), "%s: keyframe %zu bad %d / %d", tag, k, (int)a.kf[k]->isBad(), (int)b.kf[k]->isBad());
        EXPECT(a.kf[k]->mbToBeErased == b.kf[k]->mbToBeErased, "%s: keyframe %zu mbToBeErased", tag, k);
        EXPECT(a.kf[k]->N == b.kf[k]->N, "%s: keyframe %zu N", tag, k);
        for (int i = 0; i < a.kf[k]->N && i < b.kf[k]->N; i++)
            EXPECT(a.index(a.kf[k]->mvpMapPoints[i]) == b.index(b.kf[k]->mvpMapPoints[i]), "%s: keyframe %zu match %d: %d / %d", tag, k, i,
                   a.index(a.kf[k]->mvpMapPoints[i]), b.index(b.kf[k]->mvpMapPoints[i]));
    }
    for (size_t p = 0; p < a.pt.size() && p < b.pt.size(); p++) {
        EXPECT(a.pt[p]->isBad() == b.pt[p]->isBad() && a.pt[p]->nObs == b.pt[p]->nObs, "%s: point %zu bad %d / %d nObs %d / %d", tag, p, (int)a.pt[p]->isBad(),
               (int)b.pt[p]->isBad(), a.pt[p]->nObs, b.pt[p]->nObs);
        map<int, size_t> oa, ob;
        for (map<KeyFrame *, size_t>::const_iterator it = a.pt[p]->mObservations.begin(); it != a.pt[p]->mObservations.end(); ++it) oa[a.index(it->first)] = it->second;
        for (map<KeyFrame *, size_t>::const_iterator it = b.pt[p]->mObservations.begin(); it != b.pt[p]->mObservations.end(); ++it) ob[b.index(it->first)] = it->second;
        EXPECT(oa == ob, "%s: point %zu observations", tag, p);
    }
}

static map<int, int> by_index(const World &w, const map<KeyFrame *, int> &c)
{
    map<int, int> r;
    for (map<KeyFrame *, int>::const_iterator it = c.begin(); it != c.end(); ++it) r[w.index(it->first)] = it->second;
    return r;
}

static void same_votes(World &a, World &b, const char *tag)
{
    map<KeyFrame *, int> ca, cb;
    for (int k = 0; k < NK; k += 3) {
        if (a.kf[k]->isBad()) continue;
        g_hooks = true; orbx_adapter::CovisibilityCounts(a.kf[k], ca); g_hooks = false;
        host_covisibility(b.kf[k], cb);
        EXPECT(by_index(a, ca) == by_index(b, cb) && !cb.empty(), "%s: covisibility of keyframe %d (%zu / %zu entries)", tag, k, ca.size(), cb.size());
    }
    Frame fa, fb;
    fa.N = fb.N = 120;
    for (int i = 0; i < 120; i++) {
        const int p = i % 7 == 0 ? -1 : (int)rnd(NP);
        fa.mvpMapPoints.push_back(p < 0 ? NULL : a.pt[p]);
        fb.mvpMapPoints.push_back(p < 0 ? NULL : b.pt[p]);
    }
    orbx_adapter::VoteLocalKeyFrames(fa, ca);
    host_vote(fb, cb);
    EXPECT(by_index(a, ca) == by_index(b, cb) && !cb.empty(), "%s: votes (%zu / %zu entries)", tag, ca.size(), cb.size());
    for (int i = 0; i < 120; i++) EXPECT(a.index(fa.mvpMapPoints[i]) == b.index(fb.mvpMapPoints[i]), "%s: frame match %d", tag, i);
}

// more life in both maps, through the mutators: a fusion, a lost observation, a new keyframe
static void more_edits(World &w, bool hooks, bool stereo)
{
    g_hooks = hooks;
    g_rng = 777;
    for (int t = 0; t < 12; t++) {
        MapPoint *x = w.pt[rnd(NP)], *y = w.pt[rnd(NP)];
        if (!x->isBad() && !y->isBad()) x->Replace(y);
    }
    for (int t = 0; t < 25; t++) {
        MapPoint *x = w.pt[rnd(NP)];
        KeyFrame *kf = w.kf[rnd(NK)];
        if (!x->isBad() && !kf->isBad() && x->IsInKeyFrame(kf)) { const size_t i = x->mObservations[kf]; kf->EraseMapPointMatch(i); x->EraseObservation(kf); }
    }
    w.kf.push_back(w.new_kf(w.kf.size(), 30, stereo));     // (takes a slot that a culled keyframe gave back)
    KeyFrame *nk = w.kf.back();
    for (int i = 0; i < 30; i++) {
        MapPoint *x = w.pt[rnd(NP)];
        if (!x->isBad() && !x->IsInKeyFrame(nk)) { nk->AddMapPoint(x, i); x->AddObservation(nk, i); }
    }
    w.kf[NK - 1]->mvpOrderedConnectedKeyFrames.push_back(nk);
    g_hooks = false;
}

int main(int argc, char **argv)
{
    if (argc < 2 || strcmp(argv[1], "check") != 0) { fprintf(stderr, "usage: %s check [mono]\n", argv[0]); return 2; }
    const bool mono = argc > 2 && strcmp(argv[2], "mono") == 0;
    orbx_adapter::MapGraph &G = orbx_adapter::MapGraph::instance();
    try {
        World a, b;
        build(a, true, !mono, true);
        build(b, false, !mono, false);
        same_maps(a, b, "built");
        same_votes(a, b, "built");
        LocalMapping lm(mono);
        for (int round = 0; round < 2; round++) {
            int bad_before = 0, bad_after = 0, bad_pts = 0;
            for (size_t k = 0; k < b.kf.size(); k++) bad_before += b.kf[k]->isBad();
            g_hooks = true;
            lm.mpCurrentKeyFrame = a.kf[NK - 1];
            lm.KeyFrameCulling();
            g_hooks = false;
            host_culling(b.kf[NK - 1], mono);
            for (size_t k = 0; k < b.kf.size(); k++) bad_after += b.kf[k]->isBad();
            for (size_t p = 0; p < b.pt.size(); p++) bad_pts += b.pt[p]->isBad();
            same_maps(a, b, round ? "second culling" : "first culling");
            same_votes(a, b, round ? "second culling" : "first culling");
            printf("round %d culled %d to_be_erased %d bad_points %d queued %zu batches %ld echoes %ld\n", round, bad_after - bad_before, (int)b.kf[4]->mbToBeErased,
                   bad_pts, G.queued(), G.batches_sent(), G.echoes_dropped());
            EXPECT(!b.kf[0]->isBad(), "the keyframe with mnId 0 was culled");
            if (round == 0) {
                EXPECT(bad_after - bad_before >= 1 && bad_after - bad_before + (int)b.kf[4]->mbToBeErased >= 2, "the first culling culls %d keyframes: the map is too sparse for the test", bad_after - bad_before);
                more_edits(a, true, !mono);
                more_edits(b, false, !mono);
                same_maps(a, b, "more edits");
            }
        }
        g_hooks = true;
        Map m;
        m.clear();                              // Map::clear: every slot free again
        g_hooks = false;
        G.Flush();
        EXPECT(G.keyframes() == 0 && G.points() == 0, "Map::clear leaves %d keyframes, %d points", G.keyframes(), G.points());
    } catch (const std::exception &e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
    if (g_fail) { printf("%d mismatches\n", g_fail); return 1; }
    printf("adaptor mapgraph ok\n");
    return 0;
}
