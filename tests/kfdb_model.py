"""Plain-Python models of ORB_SLAM2::KeyFrameDatabase (reference src/KeyFrameDatabase.cc) and L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) for tests/test_kfdb.py.  Two independent implementations:

  RefDatabase      a line-by-line transcription: per-word posting lists, per-keyframe query / words / score members, np.float32
                   wherever the reference has `float`, Python floats for the doubles
  ForwardDatabase  the formulation the kernels use: per-pair sorted-set intersection, the (smallest common word, id) sort key and
                   the stale-score lookup, with no inverted file and no per-keyframe query state

Both expose the interface of the library's KeyFrameDatabase (ids are add sequence numbers) and the two defined deviations of
DESIGN.md section 2: every call is a fresh query identity, and mRelocScore starts at 0.0f.  The detect calls return
(candidates, words[id], score[id]) with words = the common-word count of the keyframes the query listed (0 elsewhere) and
score = the float score of the keyframes it scored (0 elsewhere)."""
import bisect

import numpy as np

F32 = np.float32


def l1_score(v1, v2):
    """ScoringObject.cpp:23-68 on two (ids, vals) vectors: the merge walk with lower_bound, one double accumulator"""
    id1, val1 = [int(x) for x in v1[0]], [float(x) for x in v1[1]]
    id2, val2 = [int(x) for x in v2[0]], [float(x) for x in v2[1]]
    i, j, score = 0, 0, 0.0
    while i < len(id1) and j < len(id2):
        vi, wi = val1[i], val2[j]
        if id1[i] == id2[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1; j += 1
        elif id1[i] < id2[j]:
            i = bisect.bisect_left(id1, id2[j])
        else:
            j = bisect.bisect_left(id2, id1[i])
    score = -score / 2.0
    return score


class _KeyFrame:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = (np.array(bow[0], np.uint32), np.array(bow[1], np.float64))
        self.mnLoopQuery = 0; self.mnLoopWords = 0; self.mLoopScore = F32(0)
        self.mnRelocQuery = 0; self.mnRelocWords = 0
        self.mRelocScore = F32(0)              # defined deviation: the reference leaves it uninitialised (src/KeyFrame.cc:35)
        self.neigh = []
        self.erased = False


class RefDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.stats = dict(gate_failed=0, groups_dropped=0, neighbour_best=0, duplicates=0, stale_nonzero=0, below_min_score=0, max_candidates=0)
        self.clear()
        self.query_id = 0                      # fresh identity per call; never 0, the value the keyframes' query members start at

    def clear(self):                           # :69-73
        self.mvInvertedFile = {}
        self.kfs = []

    def next_id(self):
        return len(self.kfs)

    def add(self, bow):                        # :40-46
        kf = _KeyFrame(len(self.kfs), bow)
        self.kfs.append(kf)
        for w in kf.mBowVec[0]:
            self.mvInvertedFile.setdefault(int(w), []).append(kf)
        return kf.mnId

    def erase(self, id):                       # :48-67
        kf = self.kfs[id]
        for w in kf.mBowVec[0]:
            lKFs = self.mvInvertedFile[int(w)]
            for k, other in enumerate(lKFs):
                if other is kf:
                    del lKFs[k]
                    break
        kf.erased = True

    def set_covisibility(self, id, neighbours):
        self.kfs[id].neigh = [int(n) for n in neighbours]

    def _best_covisibles(self, kf):            # GetBestCovisibilityKeyFrames(10): never an erased keyframe
        return [self.kfs[n] for n in kf.neigh[:10] if 0 <= n < len(self.kfs) and not self.kfs[n].erased]

    def score(self, query, ids):
        return [l1_score(query, self.kfs[i].mBowVec) for i in ids]

    def reloc_scores(self):
        return np.array([kf.mRelocScore for kf in self.kfs], np.float32)

    def _stages(self, lKFsSharingWords, words_of, scored):
        words = np.zeros(len(self.kfs), np.int32); score = np.zeros(len(self.kfs), np.float32)
        for kf in lKFsSharingWords:
            words[kf.mnId] = words_of(kf)
        for si, kf in scored:
            score[kf.mnId] = si
        return words, score

    def DetectLoopCandidates(self, bow, connected, minScore):      # :80-229
        minScore = F32(minScore)
        self.query_id += 1
        mnId = self.query_id
        spConnectedKeyFrames = set(int(c) for c in connected)
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnLoopQuery != mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        empty = ([], np.zeros(len(self.kfs), np.int32), np.zeros(len(self.kfs), np.float32))
        if not lKFsSharingWords:
            return empty
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnLoopWords > maxCommonWords:
                maxCommonWords = kf.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch, scored = [], []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F32(l1_score(bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                scored.append((si, pKFi))
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
                else:
                    self.stats["below_min_score"] += 1
            else:
                self.stats["gate_failed"] += 1
        stages = self._stages(lKFsSharingWords, lambda kf: kf.mnLoopWords, scored)
        if not lScoreAndMatch:
            return ([],) + stages
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for first, pKFi in lScoreAndMatch:
            bestScore = first; accScore = first; pBestKF = pKFi
            for pKF2 in self._best_covisibles(pKFi):
                if pKF2.mnLoopQuery == mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            if pBestKF is not pKFi:
                self.stats["neighbour_best"] += 1
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return (self._retain(lAccScoreAndMatch, bestAccScore),) + stages

    def _retain(self, lAccScoreAndMatch, bestAccScore):            # :207-228 / :330-348
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF, out = set(), []
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    out.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
                else:
                    self.stats["duplicates"] += 1
            else:
                self.stats["groups_dropped"] += 1
        self.stats["max_candidates"] = max(self.stats["max_candidates"], len(out))
        return out

    def DetectRelocalizationCandidates(self, bow):                 # :234-349
        self.query_id += 1
        mnId = self.query_id
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnRelocQuery != mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return [], np.zeros(len(self.kfs), np.int32), np.zeros(len(self.kfs), np.float32)
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
            else:
                self.stats["gate_failed"] += 1
        stages = self._stages(lKFsSharingWords, lambda kf: kf.mnRelocWords, lScoreAndMatch)
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for first, pKFi in lScoreAndMatch:
            bestScore = first; accScore = bestScore; pBestKF = pKFi
            for pKF2 in self._best_covisibles(pKFi):
                if pKF2.mnRelocQuery != mnId:
                    continue
                if not pKF2.mnRelocWords > minCommonWords and pKF2.mRelocScore != 0:
                    self.stats["stale_nonzero"] += 1
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            if pBestKF is not pKFi:
                self.stats["neighbour_best"] += 1
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return (self._retain(lAccScoreAndMatch, bestAccScore),) + stages


def forward_score(q, kf):
    """the score as the kernel forms it: the terms of the common words, added in ascending word order"""
    common, iq, ik = np.intersect1d(q[0], kf[0], assume_unique=True, return_indices=True)
    acc = 0.0
    for a, b in zip(iq, ik):
        vi, wi = float(q[1][a]), float(kf[1][b])
        acc += abs(vi - wi) - abs(vi) - abs(wi)
    return -acc / 2.0


class ForwardDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.clear()

    def clear(self):
        self.vec, self.live, self.neigh, self.persist = [], [], [], []

    def next_id(self):
        return len(self.vec)

    def add(self, bow):
        self.vec.append((np.array(bow[0], np.uint32), np.array(bow[1], np.float64)))
        self.live.append(True); self.neigh.append([]); self.persist.append(F32(0))
        return len(self.vec) - 1

    def erase(self, id):
        self.live[id] = False

    def set_covisibility(self, id, neighbours):
        self.neigh[id] = [int(n) for n in neighbours]

    def score(self, query, ids):
        return [forward_score(query, self.vec[i]) for i in ids]

    def reloc_scores(self):
        return np.array(self.persist, np.float32)

    def _count(self, bow, excluded):
        n = len(self.vec)
        words = np.zeros(n, np.int32); minw = np.zeros(n, np.int64)
        for i in range(n):
            if self.live[i] and i not in excluded:
                common = np.intersect1d(bow[0], self.vec[i][0], assume_unique=True)
                words[i] = len(common)
                minw[i] = int(common[0]) if len(common) else -1
        return words, minw

    def _query(self, bow, excluded, loop, minScore):
        n = len(self.vec)
        words, minw = self._count(bow, excluded)
        score = np.zeros(n, np.float32)
        maxCommon = int(words.max()) if n else 0
        if maxCommon == 0:
            return [], words, score
        minCommon = int(F32(maxCommon) * F32(0.8))
        scored = [i for i in range(n) if words[i] > minCommon]
        for i in scored:
            score[i] = F32(forward_score(bow, self.vec[i]))
        before = list(self.persist)
        groups = []                                      # (key, acc, best)
        best_acc = F32(minScore) if loop else F32(0)
        for i in scored:
            if loop and not score[i] >= F32(minScore):
                continue
            acc = best_s = score[i]; best = i
            for k in self.neigh[i][:10]:
                if not (0 <= k < n) or not self.live[k]:
                    continue
                if loop:
                    if not words[k] > minCommon:
                        continue
                    s2 = score[k]
                else:
                    if not words[k] > 0:
                        continue
                    s2 = score[k] if words[k] > minCommon else before[k]
                acc = F32(acc + s2)
                if s2 > best_s:
                    best, best_s = k, s2
            groups.append(((int(minw[i]), i), acc, best))
            if acc > best_acc:
                best_acc = acc
        retain = F32(F32(0.75) * best_acc)
        first = {}
        for key, acc, best in groups:
            if acc > retain and (best not in first or key < first[best]):
                first[best] = key
        if not loop:
            for i in scored:
                self.persist[i] = score[i]
        return sorted(first, key=lambda b: first[b]), words, score

    def DetectRelocalizationCandidates(self, bow):
        return self._query(bow, set(), False, 0.0)

    def DetectLoopCandidates(self, bow, connected, minScore):
        return self._query(bow, set(int(c) for c in connected), True, minScore)
