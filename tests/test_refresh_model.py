"""tests/refresh_model.py, the sequential model behind the tests of orbx_mapgraph_refresh_points, against a literal transcription of the
reference's two functions (src/MapPoint.cc:371-420 and :266-340) over dicts kept in keyframe-slot order -- the order the call states in
place of the reference's KeyFrame* address order -- and on hand cases whose answers are known without either.  No GPU."""
import numpy as np
import pytest

import refresh_model as rm
from refresh_scenes import SCALE_FACTORS, Scene


# ---- the reference's text.  A cv::Mat of CV_32F is a float32 array; cv::norm sums the squares in double; `normali / norm` scales by the
# reciprocal in double and stores floats; `normal / n` likewise (the restatement of include/orbx.h; OpenCV's own arithmetic is unpinned).

class KF:
    def __init__(self, slot, Ow, octave, desc, bad):
        self.slot, self.Ow, self.octave, self.mDescriptors, self.bad = slot, np.asarray(Ow, np.float32), octave, desc, bad
        self.mvScaleFactors, self.mnScaleLevels = SCALE_FACTORS, len(SCALE_FACTORS)

    def GetCameraCenter(self): return self.Ow.copy()
    def isBad(self): return self.bad


class MP:
    def __init__(self, pos, observations, pRefKF, bad=False):
        self.mWorldPos, self.mpRefKF, self.mbBad = np.asarray(pos, np.float32), pRefKF, bad
        self.mObservations = dict(sorted(observations.items(), key=lambda e: e[0].slot))     # std::map: ordered by key
        self.mNormalVector = self.mfMinDistance = self.mfMaxDistance = self.mDescriptor = None


def cv_norm(m):
    return np.sqrt((np.float64(m[0]) * np.float64(m[0]) + np.float64(m[1]) * np.float64(m[1])) + np.float64(m[2]) * np.float64(m[2]))


def UpdateNormalAndDepth(self):
    if self.mbBad:
        return
    observations = dict(self.mObservations)
    pRefKF = self.mpRefKF
    Pos = self.mWorldPos.copy()
    if not observations:
        return
    normal = np.zeros(3, np.float32)
    n = 0
    with np.errstate(all="ignore"):
        for pKF in observations:
            Owi = pKF.GetCameraCenter()
            normali = self.mWorldPos - Owi
            normal = normal + (normali.astype(np.float64) * (np.float64(1.0) / cv_norm(normali))).astype(np.float32)
            n += 1
        PC = Pos - pRefKF.GetCameraCenter()
        dist = np.float32(cv_norm(PC))
        level = pRefKF.octave[observations.setdefault(pRefKF, 0)]       # operator[] on the local copy
        levelScaleFactor = pRefKF.mvScaleFactors[level]
        nLevels = pRefKF.mnScaleLevels
        self.mfMaxDistance = dist * levelScaleFactor
        self.mfMinDistance = self.mfMaxDistance / pRefKF.mvScaleFactors[nLevels - 1]
        self.mNormalVector = (normal.astype(np.float64) * (np.float64(1.0) / np.float64(n))).astype(np.float32)


def DescriptorDistance(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def ComputeDistinctiveDescriptors(self):
    if self.mbBad:
        return
    observations = dict(self.mObservations)
    if not observations:
        return
    vDescriptors = []
    for pKF, idx in observations.items():
        if not pKF.isBad():
            vDescriptors.append(pKF.mDescriptors[idx])
    if not vDescriptors:
        return
    N = len(vDescriptors)
    Distances = [[0] * N for _ in range(N)]
    for i in range(N):
        Distances[i][i] = 0
        for j in range(i + 1, N):
            distij = DescriptorDistance(vDescriptors[i], vDescriptors[j])
            Distances[i][j] = distij
            Distances[j][i] = distij
    BestMedian = 2 ** 31 - 1
    BestIdx = 0
    for i in range(N):
        vDists = sorted(Distances[i])
        median = vDists[int(0.5 * (N - 1))]
        if median < BestMedian:
            BestMedian = median
            BestIdx = i
    self.mDescriptor = vDescriptors[BestIdx].copy()


def objects(sc, sg, bad=()):
    """the scene as KeyFrame / MapPoint objects of the transcription, from the slot model's rows"""
    kfs = {k: KF(k, sc.centre[k], sc.octave[k], sc.desc[k], k in bad) for k in range(sc.n_kf)}
    mps = {}
    for p, mp in sg.pt.items():
        mps[p] = MP(sc.pos[p], {kfs[kf.slot]: idx for kf, idx in mp.mObservations.items()}, kfs[int(sc.ref_kf[p])], mp.mbBad)
    return kfs, mps


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_equals_the_transcription(seed):
    sc = Scene(seed, 7, 12, 50, 8, max_row=5)
    sg = sc.model()
    sg.erase_points([3, 11])
    bad = {2, 5}
    # some reference keyframes outside the row: feature 0's octave
    for p in (4, 9, 17):
        sc.ref_kf[p] = next(k for k in range(sc.n_kf) if k not in {k for k, _ in sc.rows[p]})
    pts = list(range(sc.n_pts))
    want = sc.expect(sg, pts, 3, bad=bad)
    _, mps = objects(sc, sg, bad)
    updated = 0
    for p in pts:
        mp, w = mps[p], want[p]
        UpdateNormalAndDepth(mp)
        ComputeDistinctiveDescriptors(mp)
        assert (mp.mNormalVector is not None) == bool(w["status"] & 1), p
        assert (mp.mDescriptor is not None) == bool(w["status"] & 2), p
        if w["status"] & 1:
            assert same(mp.mNormalVector, w["geom"][4:7]) and same(mp.mfMinDistance, w["geom"][3]) and same(mp.mfMaxDistance, w["geom"][7]), p
            assert same(sc.pos[p], w["geom"][:3])
        if w["status"] & 2:
            assert np.array_equal(mp.mDescriptor, w["desc"]), p
            assert np.array_equal(sc.desc[w["best_kf"]][w["best_idx"]], w["desc"])
            updated += 1
    assert want[3]["status"] == 0 and want[11]["status"] == 0
    assert updated > 30


def two_kf_graph(n_kf=4, feats=2):
    from mapgraph_model import SlotGraph
    sg = SlotGraph(n_kf, feats, 4, 8)
    for k in range(n_kf):
        sg.set_keyframe(k, [k] + [0] * (feats - 1), [0] * feats, [0] * feats)
    return sg


def test_one_observer():
    sg = two_kf_graph()
    sg.add_observations([0], [1], [0])
    centre = {k: (0.0, 0.0, 0.0) for k in range(4)}
    centre[1] = (1.0, 2.0, -2.0)
    desc = {k: np.full((2, 32), k, np.uint8) for k in range(4)}
    r, = rm.refresh(sg, [0], 3, pos=[(1.0, 2.0, 2.0)], ref_kf=[1], centre=centre, bad={k: False for k in range(4)}, frame_desc=desc,
                    scale_factors=[1.0, 2.0, 4.0])
    assert r["status"] == 3
    # P - Ow = (0, 0, 4): the normal is the unit z, the distance 4, the octave of (kf 1, feature 0) is 1 -> max = 8, min = 8 / 4
    assert r["geom"].tolist() == [1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 1.0, 8.0]
    assert (r["best_kf"], r["best_idx"]) == (1, 0) and r["desc"].tolist() == [1] * 32


def test_two_observers_take_median_index_zero():
    """N = 2: (int)(0.5 * 1) = 0, every row's median is its own zero, the first in slot order wins whatever was added first"""
    sg = two_kf_graph()
    sg.add_observations([0, 0], [3, 2], [1, 0])
    centre = {0: (0, 0, 0), 1: (0, 0, 0), 2: (0.0, 0.0, -3.0), 3: (4.0, 0.0, 0.0)}
    desc = {k: np.full((2, 32), k, np.uint8) for k in range(4)}
    r, = rm.refresh(sg, [0], 3, pos=[(0.0, 0.0, 0.0)], ref_kf=[0], centre=centre, bad={k: False for k in range(4)}, frame_desc=desc,
                    scale_factors=[1.0, 2.0])
    # the units are (0, 0, 1) and (-1, 0, 0): the mean is (-0.5, 0, 0.5); the reference keyframe 0 is not in the row: feature 0, octave 0,
    # at distance 0
    assert r["geom"].tolist() == [0.0, 0.0, 0.0, 0.0, -0.5, 0.0, 0.5, 0.0]
    assert (r["best_kf"], r["best_idx"]) == (2, 0)


def test_tie_goes_to_the_lowest_slot_and_bad_keyframes_are_left_out():
    sg = two_kf_graph(6, 1)
    sg.add_observations([0] * 5, [5, 4, 3, 1, 0], [0] * 5)
    a, b, c = np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8), np.full(32, 0x0F, np.uint8)
    desc = {0: [a], 1: [b], 3: [c], 4: [c], 5: [b], 2: [a]}
    centre = {k: (float(k), 1.0, 1.0) for k in range(6)}
    bad = {k: k == 0 for k in range(6)}
    r, = rm.refresh(sg, [0], 2, centre=centre, bad=bad, frame_desc=desc)
    # taking part: 1 (b), 3 (c), 4 (c), 5 (b); N = 4, median index 1: b rows 0 0 128 128 -> 0, c rows 0 0 128 128 -> 0: all tie, slot 1 wins
    assert r["status"] == 2 and (r["best_kf"], r["best_idx"]) == (1, 0)
    bad[1] = bad[5] = True
    r, = rm.refresh(sg, [0], 2, centre=centre, bad=bad, frame_desc=desc)
    assert (r["best_kf"], r["best_idx"]) == (3, 0)
    r, = rm.refresh(sg, [0], 2, centre=centre, bad={k: True for k in range(6)}, frame_desc=desc)
    assert r["status"] == 0 and r["desc"] is None


def test_degenerate_distances_follow_ieee():
    sg = two_kf_graph()
    sg.add_observations([0, 0], [1, 2], [0, 0])
    centre = {0: (0, 0, 0), 1: (1.0, 1.0, 1.0), 2: (1.0, 1.0, 3.0), 3: (0, 0, 0)}
    r, = rm.refresh(sg, [0], 1, pos=[(1.0, 1.0, 1.0)], ref_kf=[1], centre=centre, scale_factors=[1.0, 2.0, 4.0])
    g = r["geom"]
    assert np.isnan(g[4:7]).all() and g[3] == 0.0 and g[7] == 0.0
