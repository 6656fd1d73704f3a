"""A sequential restatement of the reference's observation bookkeeping, on Python objects and dicts, for the tests of the resident
observation graph (orbx_mapgraph).  It follows the reference's text line by line (the citations are to its src/), keeps a MapPoint's
observations in a dict keyed by the KeyFrame object as the reference keeps them in a std::map keyed by the KeyFrame pointer, and knows
nothing of slots, rows or capacities.  SlotGraph below is the only place where slots appear: it gives the model the calls of the ABI, so
that one script of edits can drive the model and the device."""
import copy


class KeyFrame:
    def __init__(self, octave, stereo, close, mnId=1):
        n = len(octave)
        self.mnId = mnId
        self.octave = [int(o) for o in octave]           # mvKeysUn[i].octave
        self.stereo = [bool(s) for s in stereo]          # mvuRight[i] >= 0
        self.close = [bool(c) for c in close]            # 0 <= mvDepth[i] <= mThDepth
        self.mvpMapPoints = [None] * n
        self.mbNotErase = False
        self.mbToBeErased = False
        self.mbBad = False

    def AddMapPoint(self, pMP, idx):                     # src/KeyFrame.cc:222-226
        self.mvpMapPoints[idx] = pMP

    def EraseMapPointMatch(self, idx):                   # src/KeyFrame.cc:228-232
        self.mvpMapPoints[idx] = None

    def ReplaceMapPointMatch(self, idx, pMP):            # src/KeyFrame.cc:242-245
        self.mvpMapPoints[idx] = pMP

    def SetBadFlag(self):                                # src/KeyFrame.cc:489-507, the map-point part
        if self.mnId == 0:
            return
        elif self.mbNotErase:
            self.mbToBeErased = True
            return
        for i in range(len(self.mvpMapPoints)):          # :505-507, on the live vector
            if self.mvpMapPoints[i] is not None:
                self.mvpMapPoints[i].EraseObservation(self)
        self.mbBad = True


class MapPoint:
    def __init__(self, went_bad=None):
        self.mObservations = {}                          # KeyFrame -> idx
        self.nObs = 0
        self.mbBad = False
        self.went_bad = went_bad                         # the test's log of SetBadFlag calls, in order

    def AddObservation(self, pKF, idx):                  # src/MapPoint.cc:106-117
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx
        if pKF.stereo[idx]:
            self.nObs += 2
        else:
            self.nObs += 1

    def EraseObservation(self, pKF):                     # src/MapPoint.cc:119-145
        bBad = False
        if pKF in self.mObservations:
            idx = self.mObservations[pKF]
            if pKF.stereo[idx]:
                self.nObs -= 2
            else:
                self.nObs -= 1
            del self.mObservations[pKF]
            if self.nObs <= 2:
                bBad = True
        if bBad:
            self.SetBadFlag()

    def SetBadFlag(self):                                # src/MapPoint.cc:159-176
        self.mbBad = True
        obs = self.mObservations
        self.mObservations = {}
        for pKF, idx in obs.items():
            pKF.EraseMapPointMatch(idx)
        if self.went_bad is not None:
            self.went_bad.append(self)

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return self.nObs


def KeyFrameCulling(vpLocalKeyFrames, mbMonocular):
    """src/LocalMapping.cc:704-775 over the given list.  -> per keyframe of the list (mnId == 0 included, as None): (flag, nMPs,
    nRedundantObservations) with flag 0 kept / 1 SetBadFlag ran / 2 SetBadFlag left mbToBeErased"""
    out = []
    for pKF in vpLocalKeyFrames:                         # :713
        if pKF.mnId == 0:                                # :716
            out.append(None)
            continue
        vpMapPoints = list(pKF.mvpMapPoints)             # :718, a copy
        thObs = 3
        nRedundantObservations = 0
        nMPs = 0
        for i in range(len(vpMapPoints)):
            pMP = vpMapPoints[i]
            if pMP is not None:
                if not pMP.isBad():
                    if not mbMonocular:
                        if not pKF.close[i]:             # :733
                            continue
                    nMPs += 1
                    if pMP.Observations() > thObs:       # :739
                        scaleLevel = pKF.octave[i]
                        observations = dict(pMP.mObservations)
                        nObs = 0
                        for pKFi, idxi in observations.items():
                            if pKFi is pKF:
                                continue
                            scaleLeveli = pKFi.octave[idxi]
                            if scaleLeveli <= scaleLevel + 1:   # :753
                                nObs += 1
                                if nObs >= thObs:
                                    break
                        if nObs >= thObs:
                            nRedundantObservations += 1
        flag = 0
        if nRedundantObservations > 0.9 * nMPs:          # :771, int against double
            pKF.SetBadFlag()
            flag = 2 if pKF.mbToBeErased and not pKF.mbBad else 1
        out.append((flag, nMPs, nRedundantObservations))
    return out


def UpdateConnectionsCounter(pKF):
    """KFcounter of src/KeyFrame.cc:305-338"""
    KFcounter = {}
    for pMP in list(pKF.mvpMapPoints):
        if pMP is None:
            continue
        if pMP.isBad():
            continue
        for pKFi in pMP.mObservations:
            if pKFi.mnId == pKF.mnId:                    # :332
                continue
            KFcounter[pKFi] = KFcounter.get(pKFi, 0) + 1
    return KFcounter


def UpdateLocalKeyFramesCounter(vpMapPoints):
    """keyframeCounter of src/Tracking.cc:1519-1538 over a frame's mvpMapPoints"""
    keyframeCounter = {}
    for pMP in vpMapPoints:
        if pMP is not None:
            if not pMP.isBad():
                for pKFi in pMP.mObservations:
                    keyframeCounter[pKFi] = keyframeCounter.get(pKFi, 0) + 1
    return keyframeCounter


class Refused(Exception):
    def __init__(self, code):
        Exception.__init__(self, code)
        self.code = code


class SlotGraph:
    """The calls of the ABI on the model: a slot is a name for a KeyFrame / MapPoint object.  A refusal raises Refused(code) and
    leaves the model as it was.  dump() is the whole graph in the terms of orbx_mapgraph_read_keyframe / _read_points."""

    def __init__(self, max_keyframes, max_features, max_points, max_obs):
        self.lim = (max_keyframes, max_features, max_points, max_obs)
        self.clear()

    def clear(self):
        self.kf, self.pt, self.dead, self.went_bad = {}, {}, {}, []
        self.next_id = 1

    def clone(self):
        return copy.deepcopy(self)

    # -- slots
    def _kf(self, k):
        if k not in self.kf:
            raise Refused(-1)
        return self.kf[k]

    def _kf_any(self, k):          # a keyframe that may have been erased: its object lives on, as in the reference
        return self.kf.get(k) or self.dead.get(k)

    def _point(self, p, make):
        if p < 0:
            raise Refused(-1)
        if p >= self.lim[2]:
            raise Refused(-2)
        if p not in self.pt and make:
            mp = MapPoint(self.went_bad)
            mp.slot = p
            self.pt[p] = mp
        return self.pt.get(p)

    @staticmethod
    def _twice(keys):
        if len(set(keys)) != len(keys):
            raise Refused(-1)

    # -- edits
    def set_keyframe(self, k, octave, stereo, close):
        if k < 0:
            raise Refused(-1)
        if k >= self.lim[0] or len(octave) > self.lim[1]:
            raise Refused(-2)
        if k in self.kf or any(o > 31 for o in octave):
            raise Refused(-1)
        if self.keyframe_observations(k):      # observations that outlived the slot's last keyframe
            raise Refused(-1)
        kf = KeyFrame(octave, stereo, close, self.next_id)
        self.next_id += 1
        kf.slot = k
        self.kf[k] = kf
        self.dead.pop(k, None)

    def keyframe_observations(self, k):
        return sum(1 for mp in self.pt.values() for kf in mp.mObservations if kf.slot == k)

    def set_matches(self, k, idx, point):
        kf = self._kf(k)
        for i, p in zip(idx, point):
            if i < 0 or i >= len(kf.mvpMapPoints) or p < -1:
                raise Refused(-1)
            if p >= self.lim[2]:
                raise Refused(-2)
        self._twice(list(idx))
        for i, p in zip(idx, point):
            if p < 0:
                kf.EraseMapPointMatch(i)
            else:
                kf.ReplaceMapPointMatch(i, self._point(p, True))

    def add_observations(self, point, kf, idx):
        for p, k, i in zip(point, kf, idx):
            self._point(p, False)
            if i < 0 or i >= len(self._kf(k).mvpMapPoints):
                raise Refused(-1)
        self._twice(list(zip(point, kf)))
        grow = {}
        for p, k in zip(point, kf):    # a row beyond max_obs: the batch is refused whole
            mp = self.pt.get(p)
            row = set() if mp is None or mp.mbBad else set(mp.mObservations)
            s = grow.setdefault(p, row)
            s.add(self.kf[k])
            if len(s) > self.lim[3]:
                raise Refused(-2)
        for p, k, i in zip(point, kf, idx):
            mp = self._point(p, True)
            if mp.mbBad:               # the slot is used again: a new MapPoint
                del self.pt[p]
                mp = self._point(p, True)
            mp.AddObservation(self.kf[k], i)

    def erase_observations(self, point, kf):
        for p, k in zip(point, kf):
            if p < 0 or k < 0:
                raise Refused(-1)
            if p >= self.lim[2] or k >= self.lim[0]:
                raise Refused(-2)
        self._twice(list(zip(point, kf)))
        for p, k in zip(point, kf):
            mp, pKF = self.pt.get(p), self._kf_any(k)
            if mp is not None and pKF is not None:
                mp.EraseObservation(pKF)

    def erase_points(self, point):
        for p in point:
            self._point(p, False)
        self._twice(list(point))
        for p in point:
            self._point(p, True).SetBadFlag()

    def erase_keyframe(self, k):
        kf = self._kf(k)
        kf.mbNotErase = False
        kf.SetBadFlag()
        self.dead[k] = self.kf.pop(k)

    # -- queries
    def vote(self, points):
        c = UpdateLocalKeyFramesCounter([self.pt.get(p) for p in points])
        return {kf.slot: v for kf, v in c.items()}

    def covisibility(self, k):
        return {kf.slot: v for kf, v in UpdateConnectionsCounter(self._kf(k)).items()}

    def cull_keyframes(self, local, not_erase, monocular):
        kfs = [self._kf(k) for k in local]
        self._twice(list(local))
        for kf, ne in zip(kfs, not_erase):
            kf.mbNotErase, kf.mbToBeErased = bool(ne), False
        before = len(self.went_bad)
        res = KeyFrameCulling(kfs, bool(monocular))
        for k, kf, r in zip(local, kfs, res):
            kf.mbNotErase = False
            if r[0] == 1:
                self.dead[k] = self.kf.pop(k)
        return dict(culled=[r[0] for r in res], n_mps=[r[1] for r in res], n_redundant=[r[2] for r in res],
                    bad_points=sorted(mp.slot for mp in self.went_bad[before:]))

    def dump(self):
        kfs = {k: dict(point=[-1 if mp is None else mp.slot for mp in kf.mvpMapPoints], octave=kf.octave, stereo=kf.stereo, close=kf.close)
               for k, kf in self.kf.items()}
        pts = {p: dict(n_obs=mp.nObs, bad=mp.mbBad, obs=sorted((kf.slot, i) for kf, i in mp.mObservations.items()))
               for p, mp in self.pt.items() if mp.mbBad or mp.mObservations or mp.nObs}
        return kfs, pts
