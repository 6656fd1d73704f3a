// adapter/KeyFrameDatabase.cc -- the reference's src/KeyFrameDatabase.cc over orbx_kfdb_*: add / erase / clear (:40-73), DetectLoopCandidates
// (:80-229) and DetectRelocalizationCandidates (:234-349).  The query, the two gates, the L1 scores and the covisibility grouping run on the
// device; this file keeps the KeyFrame* <-> id map and hands over what only the map knows: the covisibility lists and the connected set.
#include "KeyFrameDatabase.h"

#include <stdexcept>

#include "orbx_device.h"

namespace ORB_SLAM2
{

static void flatten(const DBoW2::BowVector &v, std::vector<uint32_t> &ids, std::vector<double> &vals)
{
    ids.clear(); vals.clear();
    ids.reserve(v.size()); vals.reserve(v.size());
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) { ids.push_back((uint32_t)it->first); vals.push_back(it->second); }
}

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc) : mpDb(NULL)
{
    if (orbx_kfdb_create(orbx_adapter::Device(), (int)voc.size(), &mpDb) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
}

KeyFrameDatabase::~KeyFrameDatabase() { orbx_kfdb_destroy(mpDb); }

int KeyFrameDatabase::IdOf(KeyFrame *pKF) const
{
    std::map<long unsigned int, int>::const_iterator it = mIdOfMnId.find(pKF->mnId);
    return it == mIdOfMnId.end() ? -1 : it->second;
}

void KeyFrameDatabase::add(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (IdOf(pKF) >= 0) return;              // (the reference would list it twice in every posting list; no caller adds twice)
    std::vector<uint32_t> ids; std::vector<double> vals;
    flatten(pKF->mBowVec, ids, vals);
    int id = -1;
    if (orbx_kfdb_add(mpDb, ids.empty() ? NULL : &ids[0], vals.empty() ? NULL : &vals[0], (int)ids.size(), &id) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
    Entry e; e.pKF = pKF; e.mnId = pKF->mnId; e.sent_any = false;
    if ((int)mvEntries.size() <= id) mvEntries.resize(id + 1, Entry());
    mvEntries[id] = e;
    mIdOfMnId[pKF->mnId] = id;
}

void KeyFrameDatabase::erase(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const int id = IdOf(pKF);
    if (id < 0) return;                      // (:58-65 finds nothing to erase)
    if (orbx_kfdb_erase(mpDb, id) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
    mvEntries[id].pKF = NULL;
    mIdOfMnId.erase(pKF->mnId);
}

void KeyFrameDatabase::clear()
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (orbx_kfdb_clear(mpDb) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
    mvEntries.clear();
    mIdOfMnId.clear();
}

void KeyFrameDatabase::RefreshCovisibility()
{
    // which lists changed is not cheap to know from outside KeyFrame (UpdateBestCovisibles keeps no stamp), so every live keyframe is asked
    // and only the lists that differ from what the device holds are uploaded; neighbours the database does not hold are left out, which
    // is what the reference's lists amount to at query time (they never share a word: they are in no posting list)
    std::vector<int32_t> now;
    for (size_t id = 0; id < mvEntries.size(); id++) {
        Entry &e = mvEntries[id];
        if (!e.pKF) continue;
        const std::vector<KeyFrame *> vpNeighs = e.pKF->GetBestCovisibilityKeyFrames(10);
        now.clear();
        for (size_t k = 0; k < vpNeighs.size(); k++) {
            const int n = IdOf(vpNeighs[k]);
            if (n >= 0) now.push_back(n);
        }
        if (e.sent_any && now == e.sent) continue;
        if (orbx_kfdb_set_covisibility(mpDb, (int)id, now.empty() ? NULL : &now[0], (int)now.size()) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        e.sent = now; e.sent_any = true;
    }
}

std::vector<KeyFrame *> KeyFrameDatabase::Resolve(const std::vector<int32_t> &ids) const
{
    std::vector<KeyFrame *> out;
    out.reserve(ids.size());
    for (size_t i = 0; i < ids.size(); i++) {
        const Entry &e = mvEntries[ids[i]];
        // the record belongs to the keyframe that was added under this id: an erased one is never returned, and an address that now holds
        // another keyframe (freed without erase) is an error of the caller, not a candidate
        if (!e.pKF || e.pKF->mnId != e.mnId) throw std::logic_error("KeyFrameDatabase: a candidate's KeyFrame was freed without erase()");
        out.push_back(e.pKF);
    }
    return out;
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectLoopCandidates(KeyFrame *pKF, float minScore)
{
    const std::set<KeyFrame *> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::unique_lock<std::mutex> lock(mMutex);
    RefreshCovisibility();
    std::vector<int32_t> connected;
    for (std::set<KeyFrame *>::const_iterator it = spConnectedKeyFrames.begin(); it != spConnectedKeyFrames.end(); ++it) {
        const int id = IdOf(*it);
        if (id >= 0) connected.push_back(id);
    }
    std::vector<uint32_t> ids; std::vector<double> vals;
    flatten(pKF->mBowVec, ids, vals);
    std::vector<int32_t> cand(mvEntries.size() ? mvEntries.size() : 1);
    int ncand = 0;
    if (orbx_kfdb_detect_loop(mpDb, ids.empty() ? NULL : &ids[0], vals.empty() ? NULL : &vals[0], (int)ids.size(),
                              connected.empty() ? NULL : &connected[0], (int)connected.size(), minScore, &cand[0], (int)cand.size(), &ncand, NULL, NULL) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
    cand.resize(ncand);
    return Resolve(cand);
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)
{
    std::unique_lock<std::mutex> lock(mMutex);
    RefreshCovisibility();
    std::vector<uint32_t> ids; std::vector<double> vals;
    flatten(F->mBowVec, ids, vals);
    std::vector<int32_t> cand(mvEntries.size() ? mvEntries.size() : 1);
    int ncand = 0;
    if (orbx_kfdb_detect_relocalization(mpDb, ids.empty() ? NULL : &ids[0], vals.empty() ? NULL : &vals[0], (int)ids.size(), &cand[0], (int)cand.size(),
                                        &ncand, NULL, NULL) != ORBX_OK)
        throw std::runtime_error(orbx_last_error());
    cand.resize(ncand);
    return Resolve(cand);
}

} // namespace ORB_SLAM2
