// tests/adapter_kfdb_driver.cc -- drives ORB_SLAM2::KeyFrameDatabase (adapter/KeyFrameDatabase.cc) for tests/test_kfdb.py.
// usage: adapter_kfdb_driver <out.bin>
// Builds a small map of keyframes seen at a few places (shared base words + private ones), runs relocalisation and loop queries through the
// compiled adaptor between adds, erases, a keyframe freed and replaced, covisibility changes and a clear, and writes every input and every
// answer as a stream of events (all little-endian int32 unless noted; a vector is n, ids u32[n], values f64[n]; a list is n, int32[n]):
//   header nwords, nevents;  0 add: mnId, vector;  1 erase: mnId;  2 covisibility as it stands before a query: mnId, list of neighbour mnIds;
//   3 relocalisation: query vector, answer list (mnIds);  4 loop: query vector, connected list (mnIds), minScore f32, answer list;  5 clear
#include "KeyFrameDatabase.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

using ORB_SLAM2::KeyFrame;

static unsigned long long g_state = 88172645463325252ULL;
static unsigned rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (unsigned)(g_state >> 11); }
static double urand() { return (rnd() & 0xFFFFFF) / (double)0x1000000; }

static const int NWORDS = 50000, PLACES = 6, PER_PLACE = 6, BASE = 300, EXTRA = 80;
static std::vector<std::vector<unsigned> > g_base;

static std::string g_out;
static int g_events = 0;
static void put(const void *p, size_t n) { g_out.append((const char *)p, n); }
static void put_i(int v) { put(&v, 4); }
static void put_vec(const DBoW2::BowVector &v)
{
    put_i((int)v.size());
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) { const unsigned w = it->first; put(&w, 4); }
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) { const double x = it->second; put(&x, 8); }
}
static void put_kfs(const std::vector<KeyFrame *> &v)
{
    put_i((int)v.size());
    for (size_t i = 0; i < v.size(); i++) put_i((int)v[i]->mnId);
}

// a view of a place: 60 % of its base words plus private ones, values over three decades, L1-normalised in word order
static void view(int place, DBoW2::BowVector &out)
{
    out.clear();
    for (size_t i = 0; i < g_base[place].size(); i++)
        if (urand() < 0.6) out[g_base[place][i]] = 1.0;
    for (int i = 0; i < EXTRA; i++) out[rnd() % NWORDS] = 1.0;
    double norm = 0.0;
    for (DBoW2::BowVector::iterator it = out.begin(); it != out.end(); ++it) { it->second = pow(10.0, -3.0 * urand()); norm += it->second; }
    for (DBoW2::BowVector::iterator it = out.begin(); it != out.end(); ++it) it->second /= norm;
}

struct Map {
    std::vector<KeyFrame *> kfs;             // live in the database
    std::vector<int> place;
    ORB_SLAM2::KeyFrameDatabase *db;
    long unsigned int next_mnid;

    KeyFrame *make(int p)
    {
        KeyFrame *kf = new KeyFrame();
        kf->mnId = next_mnid; next_mnid += 3;
        view(p, kf->mBowVec);
        return kf;
    }
    void add(KeyFrame *kf, int p)
    {
        db->add(kf);
        kfs.push_back(kf); place.push_back(p);
        put_i(0); put_i((int)kf->mnId); put_vec(kf->mBowVec); g_events++;
    }
    void link(KeyFrame *kf, int p, const std::vector<KeyFrame *> &pool, const std::vector<int> &pool_place)
    {
        std::vector<KeyFrame *> same, lst;
        for (size_t i = 0; i < pool.size(); i++) if (pool[i] != kf && pool_place[i] == p) same.push_back(pool[i]);
        std::random_shuffle(same.begin(), same.end(), [](int n) { return (int)(rnd() % n); });
        for (size_t i = 0; i < same.size() && i < 4; i++) lst.push_back(same[i]);
        for (int i = 0; i < 2; i++) { KeyFrame *o = pool[rnd() % pool.size()]; if (o != kf) lst.push_back(o); }
        std::random_shuffle(lst.begin(), lst.end(), [](int n) { return (int)(rnd() % n); });
        kf->mvpOrderedConnectedKeyFrames = lst;
        kf->mConnectedKeyFrames = std::set<KeyFrame *>(lst.begin(), lst.end());
    }
    void erase(size_t i, bool free_it)
    {
        KeyFrame *kf = kfs[i];
        db->erase(kf);
        put_i(1); put_i((int)kf->mnId); g_events++;
        kfs.erase(kfs.begin() + i); place.erase(place.begin() + i);
        if (free_it) {                       // KeyFrame::SetBadFlag takes it out of every covisibility list first (src/KeyFrame.cc:468-476)
            for (size_t k = 0; k < kfs.size(); k++) {
                std::vector<KeyFrame *> &l = kfs[k]->mvpOrderedConnectedKeyFrames;
                l.erase(std::remove(l.begin(), l.end(), kf), l.end());
                kfs[k]->mConnectedKeyFrames.erase(kf);
            }
            delete kf;
        }
    }
    void dump_covisibility()
    {
        for (size_t k = 0; k < kfs.size(); k++) {
            put_i(2); put_i((int)kfs[k]->mnId); put_kfs(kfs[k]->GetBestCovisibilityKeyFrames(10)); g_events++;
        }
    }
    void reloc(int p, int second = -1)
    {
        ORB_SLAM2::Frame F;
        view(p, F.mBowVec);
        if (second >= 0) { DBoW2::BowVector b; view(second, b); for (DBoW2::BowVector::iterator it = b.begin(); it != b.end(); ++it) if (urand() < 0.5) F.mBowVec[it->first] = it->second; }
        dump_covisibility();
        const std::vector<KeyFrame *> got = db->DetectRelocalizationCandidates(&F);
        put_i(3); put_vec(F.mBowVec); put_kfs(got); g_events++;
    }
    void loop(int p, float minScore)
    {
        KeyFrame *q = make(p);
        std::vector<KeyFrame *> conn;
        for (size_t i = 0; i < kfs.size() && conn.size() < 2; i++) if (place[i] == p) conn.push_back(kfs[i]);
        conn.push_back(kfs[rnd() % kfs.size()]);
        q->mConnectedKeyFrames = std::set<KeyFrame *>(conn.begin(), conn.end());
        dump_covisibility();
        const std::vector<KeyFrame *> got = db->DetectLoopCandidates(q, minScore);
        const std::set<KeyFrame *> cs = q->GetConnectedKeyFrames();
        put_i(4); put_vec(q->mBowVec); put_kfs(std::vector<KeyFrame *>(cs.begin(), cs.end())); put(&minScore, 4); put_kfs(got); g_events++;
        delete q;
    }
};

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: adapter_kfdb_driver <out.bin>\n"); return 2; }
    g_base.resize(PLACES);
    for (int p = 0; p < PLACES; p++) for (int i = 0; i < BASE; i++) g_base[p].push_back(rnd() % NWORDS);
    ORB_SLAM2::ORBVocabulary voc(NWORDS);
    ORB_SLAM2::KeyFrameDatabase db(voc);
    Map m; m.db = &db; m.next_mnid = 100;
    for (int p = 0; p < PLACES; p++) for (int i = 0; i < PER_PLACE; i++) m.add(m.make(p), p);
    for (size_t i = 0; i < m.kfs.size(); i++) m.link(m.kfs[i], m.place[i], m.kfs, m.place);
    m.reloc(0); m.reloc(3); m.loop(3, 0.02f); m.reloc(3); m.reloc(0, 1); m.loop(5, 0.05f);
    m.erase(2, false); m.erase(19, false);   // still named by their neighbours' lists
    m.erase(7, true);                         // freed: the next keyframe may get its address, with another mnId
    m.add(m.make(1), 1);
    m.link(m.kfs.back(), 1, m.kfs, m.place);
    m.link(m.kfs[4], m.place[4], m.kfs, m.place);
    std::reverse(m.kfs[9]->mvpOrderedConnectedKeyFrames.begin(), m.kfs[9]->mvpOrderedConnectedKeyFrames.end());
    m.reloc(1); m.loop(1, 0.01f); m.reloc(0); m.reloc(3, 4); m.loop(0, 0.3f);
    db.clear(); put_i(5); g_events++;
    std::vector<KeyFrame *> old = m.kfs; std::vector<int> old_place = m.place;
    m.kfs.clear(); m.place.clear();
    for (size_t i = 0; i < 12; i++) m.add(old[i], old_place[i]);
    m.reloc(0); m.reloc(1); m.loop(1, 0.02f);

    FILE *o = fopen(argv[1], "wb");
    if (!o) { perror(argv[1]); return 2; }
    const int hdr[2] = { NWORDS, g_events };
    fwrite(hdr, 4, 2, o);
    fwrite(g_out.data(), 1, g_out.size(), o);
    fclose(o);
    return 0;
}
