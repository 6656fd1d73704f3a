// tools/kfdb_baseline.cc -- the yardstick of tools/bench_kfdb.py: place-recognition queries on ONE host core through an inverted file
// (std::vector<std::list<int>>: a posting list of keyframe indices per word), the way a CPU ORB-SLAM2 answers them.  Written for the tool
// (g++ -O3); never the code under test.  It answers with the same lists as the library (the tool checks that before it prints a time).
// usage: kfdb_baseline <scene.bin> <out.bin> <repeats>
//   scene: nwords nkf { n ids[n] vals[n] nneigh neigh[] } nq { kind n ids vals nconn conn[] min_score }     (int32 / uint32 / float64 / float32)
//   out:   per query of the first pass: ncand cand[];  then per query: best time over the passes (float64 seconds)
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <list>
#include <set>
#include <utility>
#include <vector>

struct Vec { std::vector<uint32_t> id; std::vector<double> val; };
struct Kf { Vec bow; std::vector<int> neigh; long query = -1; int words = 0; float score = 0.f; float reloc_score = 0.f; long reloc_query = -1; int reloc_words = 0; };
struct Query { int kind; Vec bow; std::vector<int> conn; float min_score; };

static std::vector<unsigned char> g_buf; static size_t g_pos = 0;
template <typename T> static T rd() { T v; std::memcpy(&v, &g_buf[g_pos], sizeof v); g_pos += sizeof v; return v; }
static void rd_vec(Vec &v)
{
    const int n = rd<int32_t>();
    v.id.resize(n); v.val.resize(n);
    for (int i = 0; i < n; i++) v.id[i] = rd<uint32_t>();
    for (int i = 0; i < n; i++) v.val[i] = rd<double>();
}

static double l1(const Vec &a, const Vec &b)
{
    size_t i = 0, j = 0; double s = 0;
    while (i < a.id.size() && j < b.id.size()) {
        if (a.id[i] == b.id[j]) { const double x = a.val[i], y = b.val[j]; s += std::fabs(x - y) - std::fabs(x) - std::fabs(y); i++; j++; }
        else if (a.id[i] < b.id[j]) i++; else j++;
    }
    return -s / 2.0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: kfdb_baseline <scene.bin> <out.bin> <repeats>\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END); g_buf.resize(std::ftell(f)); std::fseek(f, 0, SEEK_SET);
    if (std::fread(g_buf.data(), 1, g_buf.size(), f) != g_buf.size()) return 2;
    std::fclose(f);
    const int nwords = rd<int32_t>(), nkf = rd<int32_t>();
    std::vector<Kf> kfs(nkf);
    std::vector<std::list<int> > inverted(nwords);
    for (int k = 0; k < nkf; k++) {
        rd_vec(kfs[k].bow);
        const int nn = rd<int32_t>();
        for (int i = 0; i < nn; i++) kfs[k].neigh.push_back(rd<int32_t>());
        for (uint32_t w : kfs[k].bow.id) inverted[w].push_back(k);
    }
    const int nq = rd<int32_t>();
    std::vector<Query> qs(nq);
    for (Query &q : qs) {
        q.kind = rd<int32_t>(); rd_vec(q.bow);
        const int nc = rd<int32_t>();
        for (int i = 0; i < nc; i++) q.conn.push_back(rd<int32_t>());
        q.min_score = rd<float>();
    }
    const int repeats = std::atoi(argv[3]);
    std::vector<std::vector<int> > first(nq);
    std::vector<double> best(nq, 1e30);
    long stamp = 0;
    for (int pass = 0; pass < repeats; pass++)
        for (int qi = 0; qi < nq; qi++) {
            const Query &q = qs[qi];
            const auto t0 = std::chrono::steady_clock::now();
            const bool loop = q.kind == 1;
            const long me = ++stamp;
            std::set<int> conn(q.conn.begin(), q.conn.end());
            std::list<int> sharing;
            for (uint32_t w : q.bow.id)
                for (int k : inverted[w]) {
                    Kf &kf = kfs[k];
                    if (loop) {
                        if (kf.query != me) { kf.words = 0; if (!conn.count(k)) { kf.query = me; sharing.push_back(k); } }
                        kf.words++;
                    } else {
                        if (kf.reloc_query != me) { kf.reloc_words = 0; kf.reloc_query = me; sharing.push_back(k); }
                        kf.reloc_words++;
                    }
                }
            std::vector<int> out;
            if (!sharing.empty()) {
                int most = 0;
                for (int k : sharing) most = std::max(most, loop ? kfs[k].words : kfs[k].reloc_words);
                const int least = most * 0.8f;
                std::list<std::pair<float, int> > scored;
                for (int k : sharing) {
                    Kf &kf = kfs[k];
                    if ((loop ? kf.words : kf.reloc_words) > least) {
                        const float s = l1(q.bow, kf.bow);
                        if (loop) { kf.score = s; if (s >= q.min_score) scored.push_back(std::make_pair(s, k)); }
                        else { kf.reloc_score = s; scored.push_back(std::make_pair(s, k)); }
                    }
                }
                std::list<std::pair<float, int> > groups;
                float top = loop ? q.min_score : 0.f;
                for (const auto &sk : scored) {
                    float bs = sk.first, acc = sk.first; int bk = sk.second;
                    for (int n : kfs[sk.second].neigh) {
                        const Kf &o = kfs[n];
                        float s2;
                        if (loop) { if (!(o.query == me && o.words > least)) continue; s2 = o.score; }
                        else { if (o.reloc_query != me) continue; s2 = o.reloc_score; }
                        acc += s2;
                        if (s2 > bs) { bk = n; bs = s2; }
                    }
                    groups.push_back(std::make_pair(acc, bk));
                    if (acc > top) top = acc;
                }
                const float keep = 0.75f * top;
                std::set<int> seen;
                for (const auto &g : groups)
                    if (g.first > keep && !seen.count(g.second)) { out.push_back(g.second); seen.insert(g.second); }
            }
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (dt < best[qi]) best[qi] = dt;
            if (pass == 0) first[qi] = out;
        }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    for (int qi = 0; qi < nq; qi++) {
        const int32_t n = (int32_t)first[qi].size();
        std::fwrite(&n, 4, 1, o);
        for (int k : first[qi]) { const int32_t v = k; std::fwrite(&v, 4, 1, o); }
    }
    std::fwrite(best.data(), 8, nq, o);
    std::fclose(o);
    return 0;
}
