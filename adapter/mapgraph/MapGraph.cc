// adapter/mapgraph/MapGraph.cc -- see MapGraph.h
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Frame.h"
#include "LocalMapping.h"

#include <stdlib.h>
#include <stdexcept>

#include "MapGraph.h"
#include "orbx_device.h"

using namespace std;

namespace orbx_adapter
{

using ORB_SLAM2::Frame;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

static int env_int(const char *name, int otherwise)
{
    const char *env = getenv(name);
    const int v = env && *env ? atoi(env) : 0;
    return v > 0 ? v : otherwise;
}

MapGraph &MapGraph::instance()
{
    static MapGraph *g = NULL;     // never destroyed: no HIP call from a static destructor
    static std::once_flag once;
    std::call_once(once, [] {
        g = new MapGraph(env_int("ORBX_MAPGRAPH_KEYFRAMES", 4096), env_int("ORBX_MAPGRAPH_FEATURES", 4096), env_int("ORBX_MAPGRAPH_POINTS", 262144),
                         env_int("ORBX_MAPGRAPH_OBS", 256));
    });
    return *g;
}

MapGraph::MapGraph(int max_keyframes, int max_features, int max_points, int max_obs)
    : max_kf_(max_keyframes), max_feat_(max_features), max_points_(max_points), max_obs_(max_obs), graph_(NULL), kf_free_head_(0), kf_high_(0),
      pt_high_(0), batches_(0), echoes_(0)
{
}

MapGraph::~MapGraph()
{
    if (graph_) orbx_mapgraph_destroy(graph_);
}

static thread_local int t_echo = 0;
MapGraph::EchoScope::EchoScope() { t_echo++; }
MapGraph::EchoScope::~EchoScope() { t_echo--; }

// the caller holds mu_
bool MapGraph::echo()
{
    if (!t_echo) return false;
    echoes_++;
    return true;
}

void MapGraph::check(int rc)
{
    if (rc != ORBX_OK) throw std::runtime_error(orbx_last_error());
}

orbx_mapgraph *MapGraph::graph()
{
    if (!graph_) check(orbx_mapgraph_create(Device(), max_kf_, max_feat_, max_points_, max_obs_, &graph_));
    return graph_;
}

// ---- slots (the caller holds mu_)

void MapGraph::give_up_keyframe(KeyFrame *pKF, bool queue)
{
    unordered_map<KeyFrame *, Id>::iterator it = kf_.find(pKF);
    if (it == kf_.end()) return;
    if (queue) queue_.push_back(Rec{ ERASE_KEYFRAME, it->second.slot, 0, 0 });
    kf_free_.push_back(it->second.slot);
    kf_.erase(it);
}

int MapGraph::kf_slot(KeyFrame *pKF)
{
    unordered_map<KeyFrame *, Id>::iterator it = kf_.find(pKF);
    if (it == kf_.end()) return -1;
    if (it->second.id != pKF->mnId) {      // another keyframe at a known address: the one we knew is gone, without SetBadFlag
        give_up_keyframe(pKF, true);
        return -1;
    }
    return it->second.slot;
}

int MapGraph::point_slot(MapPoint *pMP, bool make)
{
    unordered_map<MapPoint *, Id>::iterator it = pt_.find(pMP);
    if (it != pt_.end()) {
        if (it->second.id == pMP->mnId) return it->second.slot;
        if (!pt_bad_[it->second.slot]) {   // another point at a known address
            pt_bad_[it->second.slot] = 1;
            queue_.push_back(Rec{ ERASE_POINT, it->second.slot, 0, 0 });
        }
        pt_.erase(it);
    }
    if (!make) return -1;
    if (pt_high_ >= max_points_) throw std::runtime_error("orbx_adapter::MapGraph: out of point slots (ORBX_MAPGRAPH_POINTS)");
    const int s = pt_high_++;
    if (pt_bad_.size() <= (size_t)s) pt_bad_.resize((size_t)s + 1024, 0);
    pt_bad_[s] = 0;
    pt_[pMP] = Id{ s, pMP->mnId };
    return s;
}

// ---- hooks

void MapGraph::OnNewKeyFrame(KeyFrame *pKF)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (echo()) return;
    give_up_keyframe(pKF, true);           // whatever lived at this address before
    const int n = pKF->N;
    if (n > max_feat_) throw std::runtime_error("orbx_adapter::MapGraph: a keyframe with more features than ORBX_MAPGRAPH_FEATURES");
    // a free slot that no observation names any more (an observation without a match outlives its keyframe, as a pointer to a bad KeyFrame
    // does in the reference; the library's count lags the queue on the safe side), or a new one
    int s = -1;
    for (size_t tries = kf_free_.size() - kf_free_head_ < 8 ? kf_free_.size() - kf_free_head_ : 8; tries > 0 && s < 0; tries--) {
        const int cand = kf_free_[kf_free_head_++];
        if (graph_ && orbx_mapgraph_keyframe_observations(graph_, cand) != 0) kf_free_.push_back(cand); else s = cand;
    }
    if (kf_free_head_ > 1024 && 2 * kf_free_head_ > kf_free_.size()) { kf_free_.erase(kf_free_.begin(), kf_free_.begin() + (long)kf_free_head_); kf_free_head_ = 0; }
    if (s < 0) {
        if (kf_high_ >= max_kf_) throw std::runtime_error("orbx_adapter::MapGraph: out of keyframe slots (ORBX_MAPGRAPH_KEYFRAMES)");
        s = kf_high_++;
    }
    if (kf_of_slot_.size() <= (size_t)s) kf_of_slot_.resize((size_t)s + 64, NULL);
    kf_of_slot_[s] = pKF;
    kf_[pKF] = Id{ s, pKF->mnId };
    queue_.push_back(Rec{ SET_KEYFRAME, s, (int32_t)attr_.size(), n });
    const size_t at = attr_.size();
    attr_.resize(at + 3 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const int oct = pKF->mvKeysUn[i].octave;
        attr_[at + i] = (unsigned char)(oct < 0 ? 0 : oct > 31 ? 31 : oct);
        attr_[at + n + i] = pKF->mvuRight[i] >= 0 ? 1 : 0;
        attr_[at + 2 * n + i] = pKF->mvDepth[i] >= 0 && pKF->mvDepth[i] <= pKF->mThDepth ? 1 : 0;   // src/LocalMapping.cc:733, negated
    }
}

void MapGraph::OnSetMatch(KeyFrame *pKF, size_t idx, MapPoint *pMP)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (echo()) return;
    const int k = kf_slot(pKF);
    if (k < 0) { echoes_++; return; }      // a keyframe the graph has given up already
    queue_.push_back(Rec{ SET_MATCH, k, (int32_t)idx, pMP ? point_slot(pMP, true) : -1 });
}

void MapGraph::OnKeyFrameBad(KeyFrame *pKF)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (echo()) return;
    if (kf_slot(pKF) < 0) { echoes_++; return; }
    give_up_keyframe(pKF, true);
}

void MapGraph::OnAddObservation(MapPoint *pMP, KeyFrame *pKF, size_t idx)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (echo()) return;
    const int k = kf_slot(pKF);
    if (k < 0) { echoes_++; return; }
    queue_.push_back(Rec{ ADD_OBS, point_slot(pMP, true), k, (int32_t)idx });
}

void MapGraph::OnEraseObservation(MapPoint *pMP, KeyFrame *pKF)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (echo()) return;
    const int k = kf_slot(pKF), p = point_slot(pMP, false);
    if (k < 0 || p < 0) { echoes_++; return; }      // KeyFrame::SetBadFlag's own loop, behind OnKeyFrameBad: the graph has done it
    queue_.push_back(Rec{ ERASE_OBS, p, k, 0 });
}

void MapGraph::OnPointBad(MapPoint *pMP)
{
    std::lock_guard<std::mutex> lk(mu_);
    if (echo()) return;
    const int p = point_slot(pMP, false);
    if (p < 0) return;
    if (!pt_bad_[p]) { pt_bad_[p] = 1; queue_.push_back(Rec{ ERASE_POINT, p, 0, 0 }); }
    // (a point that an EraseObservation took to nObs <= 2 arrives here too: the graph has made it bad by itself, and erasing a bad point
    // again changes nothing)
    pt_.erase(pMP);
}

void MapGraph::OnMapClear()
{
    std::lock_guard<std::mutex> lk(mu_);
    queue_.clear(); attr_.clear();
    queue_.push_back(Rec{ CLEAR, 0, 0, 0 });
    kf_.clear(); pt_.clear(); kf_free_.clear(); kf_free_head_ = 0; kf_high_ = 0; pt_high_ = 0;
    kf_of_slot_.assign(kf_of_slot_.size(), NULL);
}

// ---- the queue

void MapGraph::flush_locked()
{
    if (queue_.empty()) return;
    orbx_mapgraph *g = graph();
    vector<int32_t> a, b, c;
    size_t i = 0;
    try {
        while (i < queue_.size()) {
            const Rec &r = queue_[i];
            size_t j = i + 1;
            switch (r.kind) {
            case CLEAR: check(orbx_mapgraph_clear(g)); break;
            case SET_KEYFRAME: {
                const unsigned char none = 0;
                const unsigned char *at = r.c ? &attr_[(size_t)r.b] : &none;
                check(orbx_mapgraph_set_keyframe(g, r.a, r.c, at, at + r.c, at + 2 * r.c));
                break;
            }
            case ERASE_KEYFRAME: check(orbx_mapgraph_erase_keyframe(g, r.a)); break;
            case SET_MATCH:
            case ADD_OBS: {
                // AddMapPoint and AddObservation come interleaved, and commute: one touches the keyframe view only, the other reads no
                // match.  The run of both kinds in which no key comes twice travels as one add_observations and one set_matches per keyframe
                // (a key named twice in a batch is refused by the ABI, and its two records must be applied in order anyway).
                a.clear(); b.clear(); c.clear();
                vector<Rec> ms;
                for (j = i; j < queue_.size(); j++) {
                    const Rec &q = queue_[j];
                    if (q.kind != SET_MATCH && q.kind != ADD_OBS) break;
                    bool twice = false;
                    if (q.kind == SET_MATCH) for (size_t t = 0; t < ms.size() && !twice; t++) twice = ms[t].a == q.a && ms[t].b == q.b;
                    else for (size_t t = 0; t < a.size() && !twice; t++) twice = a[t] == q.a && b[t] == q.b;
                    if (twice) break;
                    if (q.kind == SET_MATCH) ms.push_back(q); else { a.push_back(q.a); b.push_back(q.b); c.push_back(q.c); }
                }
                if (!a.empty()) { check(orbx_mapgraph_add_observations(g, &a[0], &b[0], &c[0], (int)a.size())); batches_++; }
                vector<char> done(ms.size(), 0);
                for (size_t t = 0; t < ms.size(); t++) {
                    if (done[t]) continue;
                    b.clear(); c.clear();
                    for (size_t u = t; u < ms.size(); u++)
                        if (!done[u] && ms[u].a == ms[t].a) { b.push_back(ms[u].b); c.push_back(ms[u].c); done[u] = 1; }
                    check(orbx_mapgraph_set_matches(g, ms[t].a, &b[0], &c[0], (int)b.size()));
                    batches_++;
                }
                batches_--;
                break;
            }
            default: {
                // the run of records of this kind in which no key comes twice
                a.clear(); b.clear();
                for (j = i; j < queue_.size(); j++) {
                    const Rec &q = queue_[j];
                    if (q.kind != r.kind) break;
                    bool twice = false;
                    for (size_t t = 0; t < a.size() && !twice; t++) twice = a[t] == q.a && (r.kind == ERASE_POINT || b[t] == q.b);
                    if (twice) break;
                    a.push_back(q.a); b.push_back(q.b);
                }
                if (r.kind == ERASE_OBS) check(orbx_mapgraph_erase_observations(g, &a[0], &b[0], (int)a.size()));
                else check(orbx_mapgraph_erase_points(g, &a[0], (int)a.size()));
            }
            }
            batches_++;
            i = j;
        }
    } catch (...) {
        queue_.erase(queue_.begin(), queue_.begin() + (long)i);    // what has been sent stays sent
        throw;
    }
    queue_.clear(); attr_.clear();
}

void MapGraph::Flush()
{
    std::lock_guard<std::mutex> lk(mu_);
    flush_locked();
}

bool MapGraph::Knows(KeyFrame *pKF)
{
    std::lock_guard<std::mutex> lk(mu_);
    return kf_slot(pKF) >= 0;
}

int MapGraph::keyframes() { std::lock_guard<std::mutex> lk(mu_); return (int)kf_.size(); }
int MapGraph::points() { std::lock_guard<std::mutex> lk(mu_); return pt_high_; }
size_t MapGraph::queued() { std::lock_guard<std::mutex> lk(mu_); return queue_.size(); }
long MapGraph::batches_sent() { std::lock_guard<std::mutex> lk(mu_); return batches_; }
long MapGraph::echoes_dropped() { std::lock_guard<std::mutex> lk(mu_); return echoes_; }

void MapGraph::Cull(const vector<KeyFrame *> &local, bool monocular, vector<unsigned char> &flag)
{
    std::lock_guard<std::mutex> lk(mu_);
    const size_t n = local.size();
    vector<int32_t> slots(n);
    vector<unsigned char> not_erase(n);
    for (size_t j = 0; j < n; j++) {
        slots[j] = kf_slot(local[j]);
        if (slots[j] < 0) throw std::runtime_error("orbx_adapter::MapGraph::Cull: a keyframe without a slot");
        not_erase[j] = local[j]->GetNotErase() ? 1 : 0;
    }
    flush_locked();
    flag.assign(n, 0);
    if (n == 0) return;
    vector<int32_t> bad((size_t)pt_high_ + 1);
    int n_bad = 0;
    check(orbx_mapgraph_cull_keyframes(graph(), &slots[0], &not_erase[0], (int)n, monocular ? 1 : 0, &flag[0], NULL, NULL, &bad[0], (int)bad.size(), &n_bad));
    // what the graph has applied itself: the culled keyframes' slots are free, their bad points are bad
    for (size_t j = 0; j < n; j++)
        if (flag[j] == 1) give_up_keyframe(local[j], false);
    for (int t = 0; t < n_bad; t++) pt_bad_[bad[t]] = 1;
}

} // namespace orbx_adapter

namespace ORB_SLAM2
{

// One orbx_mapgraph_cull_keyframes call for the whole loop of src/LocalMapping.cc:713-774, then SetBadFlag on the culled keyframes in the
// loop's order for everything that is not the graph's (connections, spanning tree, mbToBeErased, the map and the database): the hooks
// that those calls fire repeat what the graph has applied between its iterations, and are dropped.
void LocalMapping::KeyFrameCulling()
{
    orbx_adapter::MapGraph &G = orbx_adapter::MapGraph::instance();
    const vector<KeyFrame *> vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();
    vector<KeyFrame *> local;
    for (size_t j = 0; j < vpLocalKeyFrames.size(); j++)
        if (vpLocalKeyFrames[j]->mnId != 0 && G.Knows(vpLocalKeyFrames[j])) local.push_back(vpLocalKeyFrames[j]);
    vector<unsigned char> flag;
    G.Cull(local, mbMonocular, flag);
    orbx_adapter::MapGraph::EchoScope echoes;
    for (size_t j = 0; j < local.size(); j++)
        if (flag[j]) local[j]->SetBadFlag();
}

} // namespace ORB_SLAM2

namespace orbx_adapter
{

void CovisibilityCounts(KeyFrame *pKF, map<KeyFrame *, int> &KFcounter)
{
    MapGraph &G = MapGraph::instance();
    std::lock_guard<std::mutex> lk(G.mu_);
    KFcounter.clear();
    const int k = G.kf_slot(pKF);
    if (k < 0) throw std::runtime_error("orbx_adapter::CovisibilityCounts: a keyframe without a slot");
    G.flush_locked();
    vector<int32_t> counts((size_t)G.max_kf_), nz((size_t)G.max_kf_);
    int n = 0;
    G.check(orbx_mapgraph_covisibility(G.graph(), k, &counts[0], &nz[0], &n));
    for (int t = 0; t < n; t++)
        if ((size_t)nz[t] < G.kf_of_slot_.size() && G.kf_of_slot_[nz[t]]) KFcounter[G.kf_of_slot_[nz[t]]] = counts[nz[t]];
}

void VoteLocalKeyFrames(Frame &F, map<KeyFrame *, int> &keyframeCounter)
{
    MapGraph &G = MapGraph::instance();
    std::lock_guard<std::mutex> lk(G.mu_);
    keyframeCounter.clear();
    vector<int32_t> pts;
    for (int i = 0; i < F.N; i++) {
        MapPoint *pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad()) { F.mvpMapPoints[i] = NULL; continue; }      // src/Tracking.cc:1533-1536
        const int p = G.point_slot(pMP, false);
        if (p >= 0) pts.push_back(p);
    }
    G.flush_locked();
    if (pts.empty()) return;
    vector<int32_t> counts((size_t)G.max_kf_), nz((size_t)G.max_kf_);
    int n = 0;
    G.check(orbx_mapgraph_vote(G.graph(), &pts[0], (int)pts.size(), &counts[0], &nz[0], &n));
    for (int t = 0; t < n; t++)
        if ((size_t)nz[t] < G.kf_of_slot_.size() && G.kf_of_slot_[nz[t]]) keyframeCounter[G.kf_of_slot_[nz[t]]] = counts[nz[t]];
}

} // namespace orbx_adapter
