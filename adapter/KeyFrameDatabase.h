// adapter/KeyFrameDatabase.h -- ORB_SLAM2::KeyFrameDatabase with the reference's public interface (include/KeyFrameDatabase.h:42-70) over
// orbx_kfdb_* (include/orbx.h): replaces the reference's include/KeyFrameDatabase.h + src/KeyFrameDatabase.cc.  The BowVectors live in HBM after
// add(); the inverted file is gone (the reference's candidate order is a function of the data).
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"
#include "orbx.h"

namespace ORB_SLAM2
{

class KeyFrame;
class Frame;

class KeyFrameDatabase
{
public:
    KeyFrameDatabase(const ORBVocabulary &voc);
    ~KeyFrameDatabase();

    void add(KeyFrame *pKF);
    void erase(KeyFrame *pKF);
    void clear();

    // Loop Detection
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore);
    // Relocalization
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F);

protected:
    // one record per database id (the add sequence number).  A keyframe is known by its mnId, never by its address alone: a KeyFrame freed
    // and another allocated at the same address must not inherit the record (the hazard ADVICE.md describes for KeyFrameCache)
    struct Entry {
        KeyFrame *pKF;                      // NULL once erased
        long unsigned int mnId;
        std::vector<int32_t> sent;          // the neighbour ids last handed to orbx_kfdb_set_covisibility
        bool sent_any;
    };
    int IdOf(KeyFrame *pKF) const;          // database id, or -1
    // GetBestCovisibilityKeyFrames(10) of every live keyframe; uploads the lists that changed, one small synchronous copy each under mMutex:
    // a handful per query in steady state, one per keyframe on the first query after a bulk load (an ABI call that takes many lists at
    // once is the follow-up if that first query matters)
    void RefreshCovisibility();
    std::vector<KeyFrame *> Resolve(const std::vector<int32_t> &ids) const;

    orbx_kfdb *mpDb;
    std::vector<Entry> mvEntries;
    std::map<long unsigned int, int> mIdOfMnId;
    std::mutex mMutex;
};

} // namespace ORB_SLAM2

#endif
