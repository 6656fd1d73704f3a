"""The window walk that k_proj_lists and k_window_best share (orbx_proj.hip: window_walk) on its smallest hard input: one workgroup of
four points against a 640x480 frame (cells of 10x10 px) whose features sit in one 30x30 px patch -- three grid columns, three rows, 200
features, so the flattened candidate sequence takes four 64-candidate chunks and the first column's run crosses a chunk boundary.  The
same scene goes through every search that builds candidate lists (k_proj_lists: host-pointer and resident forms) and through the
resident window-best calls (k_window_best), so both visitors of the walk meet the same input; every result equals the CPU oracle's."""
import functools

import numpy as np
import pytest

from test_kf_resident import _frame_only, _windows
from test_projection import POP

f32 = np.float32
SF = np.array([f32(1.2) ** i for i in range(8)], f32)
INV_S2 = (1.0 / (SF * SF)).astype(f32)
TH = 14.0            # radius 14 * 1.2 = 16.8 px at level 1: cells 29..33 x 19..23 around (310, 210), the whole patch inside the box
TH_MAP = 5.5         # the map-point search: 2.5 * 5.5 * 1.2 = 16.5 px
PER_COLUMN = (90, 70, 40)     # features in grid columns 30, 31, 32 (x in [295, 305), [305, 315), [315, 325))
SETTINGS = ("ties", "two_minima")


def _flip(desc, rng, nbits):
    out = desc.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


@functools.lru_cache(maxsize=None)
def _scene(setting):
    """-> (frame, points, walk): walk = the features of point 0's window cells in GetFeaturesInArea's traversal order"""
    rng = np.random.Generator(np.random.PCG64(2024))
    xs, ys = [], []
    for c, m in enumerate(PER_COLUMN):
        xs.append(295.25 + 10 * c + 9.5 * rng.random(m))
        ys.append(195.25 + 29.5 * rng.random(m) ** 2)                    # uneven over the rows 20, 21, 22
    npatch = sum(PER_COLUMN)
    nfar = 12
    x = np.concatenate(xs + [rng.uniform(20, 250, nfar)]); y = np.concatenate(ys + [rng.uniform(20, 150, nfar)])
    n = npatch + nfar
    perm = rng.permutation(n)                                            # feature numbers unrelated to the position
    x = x[perm].astype(f32); y = y[perm].astype(f32)
    patch = perm < npatch
    octave = np.where(patch, rng.choice([0, 1, 1, 1, 2, 3], n), 1).astype(np.int32)
    qdesc = rng.integers(0, 256, 32, dtype=np.uint8)                     # the descriptor of every point
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    frame = dict(x=x, y=y, octave=octave, angle=np.zeros(n, f32), u_right=np.full(n, -1, f32), desc=desc, occupied=np.zeros(n, np.uint8),
                 bounds=(0.0, 0.0, 640.0, 480.0))
    #        centred on the patch, window without a feature, outside the image, invalid (on the patch)
    pts = dict(u=np.array([310, 100, 700, 310], f32), v=np.array([210, 400, 210, 210], f32), aux=np.full(4, 0.1, f32),
               level=np.ones(4, np.int32), angle=np.zeros(4, f32), view_cos=np.ones(4, f32), desc=np.repeat(qdesc[None], 4, axis=0),
               valid=np.array([1, 1, 1, 0], np.uint8), has_obs=np.ones(4, np.uint8))
    px = np.floor(x * f32(0.1) + f32(0.5)).astype(np.int64); py = np.floor(y * f32(0.1) + f32(0.5)).astype(np.int64)
    in_win = (px >= 29) & (px <= 33) & (py >= 19) & (py <= 23)
    order = np.lexsort((np.arange(n), py, px))
    walk = order[in_win[order]]
    if setting == "ties":
        desc[patch] = qdesc                                              # every patch feature at distance 0
    else:
        for k in np.nonzero(patch)[0]:
            desc[k] = _flip(qdesc, rng, int(rng.integers(20, 61)))
        level1 = [int(p) for p in range(len(walk)) if octave[walk[p]] == 1]
        p1 = [p for p in level1 if p < 64][5]; p3 = [p for p in level1 if 128 <= p < 192][5]
        desc[walk[p1]] = _flip(qdesc, rng, 5); desc[walk[p3]] = _flip(qdesc, rng, 5)   # the minimum twice: first and third chunk
    for a in list(frame.values()) + list(pts.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return frame, pts, walk


def _check_scene(oracle, setting):
    """the properties the test rests on, from the scene and the oracle alone; -> the oracle's answers, computed once per setting"""
    frame, pts, walk = _scene(setting)
    px = np.floor(frame["x"] * f32(0.1) + f32(0.5)).astype(np.int64); py = np.floor(frame["y"] * f32(0.1) + f32(0.5)).astype(np.int64)
    assert len(walk) == sum(PER_COLUMN) >= 3 * 64 and len(frame["x"]) > len(walk)            # four chunks; a handful of features elsewhere
    runs = np.array([(px[walk] == c).sum() for c in range(29, 34)])
    assert list(runs) == [0] + list(PER_COLUMN) + [0]
    ends = np.cumsum(runs); begs = ends - runs
    assert any(b < 64 * m < e for b, e in zip(begs, ends) for m in (1, 2, 3))                # a column's run crosses a chunk boundary
    rows = [int((py[walk] == r).sum()) for r in (20, 21, 22)]
    print(setting, "columns", [int(c) for c in runs], "rows", rows)
    assert sum(rows) == len(walk) and min(rows) >= 10 and max(rows) >= 2 * min(rows)         # uneven over three rows
    in_cells, at_best, first = _windows(frame, pts, SF, TH, 100)
    assert list(in_cells) == [len(walk), 0, 0, 0]                       # point 1's window is empty, point 2 is outside, point 3 invalid
    d = POP[frame["desc"][walk] ^ pts["desc"][0]].sum(axis=1)
    ok = (frame["octave"][walk] >= 0) & (frame["octave"][walk] <= 1)
    if setting == "ties":
        assert (d == 0).all() and at_best[0] == ok.sum() >= 100 and first[0] == walk[ok][0]
    else:
        pos = np.nonzero(d == d.min())[0]
        assert d.min() == 5 and len(pos) == 2 and pos[0] < 64 and 128 <= pos[1] < 192 and ok[pos].all()
        assert at_best[0] == 2 and first[0] == walk[pos[0]]
    if setting not in _ORACLE:
        p_far = dict(pts, aux=(pts["u"] - 8).astype(f32))
        _ORACLE[setting] = dict(
            last=[oracle.search_by_projection_last(frame, pts, SF, TH, direction, 0.0, True) for direction in (0, 1, 2)],
            points=oracle.search_by_projection_points(frame, pts, SF, TH_MAP, 0.9),
            keyframe=oracle.search_by_projection_keyframe(frame, pts, SF, TH, 100, True),
            sim3=oracle.search_by_projection_sim3(frame, pts, SF, TH),
            best=oracle.window_best(frame, pts, SF, INV_S2, TH, 0, 100),
            best_chi2=oracle.window_best(frame, p_far, SF, INV_S2, TH, 1, 50))
    exp = _ORACLE[setting]

    def winner(lo, hi):                                                  # the first candidate at the minimum among the levels [lo, hi]
        adm = (frame["octave"][walk] >= lo) & (frame["octave"][walk] <= hi)
        return walk[adm][np.argmin(d[adm])]

    assert exp["best"][0][0] == first[0] == winner(0, 1) and list(exp["best"][0][1:]) == [-1, -1, -1] and exp["best"][2] == 1
    assert exp["best_chi2"][2] == 1 and exp["best_chi2"][0][0] != exp["best"][0][0]          # the chi2 gate bites: another winner
    ranges = [(0, 2), (1, 7), (0, 1), (0, 1), (0, 2), (0, 1)]           # last frame: none / forward / backward, map points, keyframe, Sim3
    for (m, nm), (lo, hi), what in zip(exp["last"] + [exp["points"], exp["keyframe"], exp["sim3"]], ranges, range(6)):
        if what == 3 and setting == "two_minima":                        # two equal minima on one level: the map-point ratio test refuses
            assert nm == 0 and (m == -1).all()
        else:
            assert nm == 1 and m[winner(lo, hi)] == 0 and (m >= 0).sum() == 1, what
    return exp


_ORACLE = {}


@pytest.mark.parametrize("setting", SETTINGS)
def test_scene_and_oracle(oracle, setting):
    _check_scene(oracle, setting)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS)
def test_walk_both_visitors(pkg, oracle, setting):
    exp = _check_scene(oracle, setting)
    frame, pts, _ = _scene(setting)
    p_far = dict(pts, aux=(pts["u"] - 8).astype(f32))
    occ = frame["occupied"]
    mt, mr = pkg.ORBmatcher(0.9, True), pkg.ORBmatcher(0.9, True)
    kf = pkg.DeviceFrame(_frame_only(frame))

    def same(got, want, what):
        assert len(got) == len(want), what
        for g, w in zip(got, want):
            assert np.array_equal(np.asarray(g), np.asarray(w)), (setting, what, g, w)

    # ---- k_proj_lists: the host-pointer searches and their resident forms
    for direction, want in zip((0, 1, 2), exp["last"]):
        same(mt.SearchByProjectionLastFrame(frame, pts, SF, TH, direction, 0.0), want, ("last", direction))
        same(mr.SearchByProjectionLastFrameResident(kf, occ, pts, SF, TH, direction, 0.0), want, ("last resident", direction))
    same(mt.SearchByProjectionMapPoints(frame, pts, SF, TH_MAP), exp["points"], "points")
    same(mr.SearchByProjectionMapPointsResident(kf, occ, pts, SF, TH_MAP), exp["points"], "points resident")
    same(mt.SearchByProjectionKeyFrame(frame, pts, SF, TH, 100), exp["keyframe"], "keyframe")
    same(mr.SearchByProjectionKeyFrameResident(kf, occ, pts, SF, TH, 100), exp["keyframe"], "keyframe resident")
    same(mt.SearchByProjectionSim3(frame, pts, SF, TH), exp["sim3"], "sim3")
    same(mr.SearchByProjectionSim3Resident(kf, occ, pts, SF, TH), exp["sim3"], "sim3 resident")
    same(mt.Fuse(frame, pts, SF, None, TH, 100), exp["best"], "window_best")
    same(mt.Fuse(frame, p_far, SF, INV_S2, TH, 50), exp["best_chi2"], "window_best chi2")
    # ---- k_window_best: the resident window-best call and a two-job batch
    same(mr.FuseResident(kf, pts, SF, None, TH, 100), exp["best"], "window_best resident")
    res = mr.FuseResidentBatch([dict(kf=kf, points=pts, scaleFactors=SF, th=TH, max_dist=100),
                                dict(kf=kf, points=p_far, scaleFactors=SF, invLevelSigma2=INV_S2, th=TH, max_dist=50)])
    same(res[0], exp["best"], "batch job 0")
    same(res[1], exp["best_chi2"], "batch job 1")
