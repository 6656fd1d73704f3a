"""Maps for the tests of the resident observation graph: a Scene is a script of the ABI's edits, played into the model's SlotGraph
(tests/mapgraph_model.py) and into the device's MapGraph alike.  CULL_CASES are the hand-built maps of KeyFrameCulling with their
expected values written out by hand; random_cull_scene / random_edit_batches are the seeded generators."""
import numpy as np


class Scene:
    def __init__(self):
        self.ops, self.nfeat = [], {}
        self._m, self._o = {}, []
        self.top_point = -1

    # -- building
    def kf(self, k, n, octave=0, stereo=False, close=True):
        """a keyframe of n features; octave / stereo / close: one value for all features, or a list"""
        self._flush()
        col = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n
        self.ops.append(("set_keyframe", (k, [int(x) for x in col(octave)], [int(bool(x)) for x in col(stereo)], [int(bool(x)) for x in col(close)])))
        self.nfeat[k] = n

    def match(self, k, i, p):
        """KeyFrame::AddMapPoint alone"""
        self._m.setdefault(k, {})[i] = p
        self.top_point = max(self.top_point, p)

    def obs(self, p, k, i):
        """MapPoint::AddObservation alone"""
        self._o.append((p, k, i))
        self.top_point = max(self.top_point, p)

    def see(self, p, k, i):
        """keyframe k observes point p at feature i: both views"""
        self.match(k, i, p)
        self.obs(p, k, i)

    def op(self, name, *args):
        self._flush()
        self.ops.append((name, args))

    def _flush(self):
        for k, m in self._m.items():
            self.ops.append(("set_matches", (k, list(m.keys()), list(m.values()))))
        if self._o:
            self.ops.append(("add_observations", tuple([list(c) for c in zip(*self._o)])))
        self._m, self._o = {}, []

    # -- playing
    def limits(self, max_obs=8):
        self._flush()
        return (max(self.nfeat) + 1, max(max(self.nfeat.values()), 1), self.top_point + 2, max_obs)

    def play(self, g):
        self._flush()
        for name, args in self.ops:
            getattr(g, name)(*args)
        return g


def _observers(s, first, n, nfeat, octave=0, stereo=False):
    """helper keyframes first .. first + n - 1 that the culling loop never judges"""
    for k in range(first, first + n):
        s.kf(k, nfeat, octave=octave, stereo=stereo)


def _scale(octs, name, expect):
    # keyframe 0 holds point 0 at octave 2; keyframes 1-3 observe it at the octaves `octs`
    s = Scene()
    s.kf(0, 1, octave=2)
    for k, o in zip((1, 2, 3), octs):
        s.kf(k, 1, octave=o)
    for k in range(4):
        s.see(0, k, 0)
    return dict(name=name, scene=s, local=[0], not_erase=[0], monocular=True, expect=expect)


def _nobs(weights, name, expect, own=False):
    # point 0 is matched in keyframe 0 (observed by it only when `own`); keyframes 1.. observe it, stereo where the weight is 2
    s = Scene()
    s.kf(0, 1, stereo=own == 2)
    for k, w in enumerate(weights, 1):
        s.kf(k, 1, stereo=w == 2)
    if own:
        s.see(0, 0, 0)
    else:
        s.match(0, 0, 0)
    for k in range(1, len(weights) + 1):
        s.see(0, k, 0)
    return dict(name=name, scene=s, local=[0], not_erase=[0], monocular=True, expect=expect)


def _far(mono, name, expect):
    # keyframe 0: feature 0 far, feature 1 close, both points seen by three more keyframes
    s = Scene()
    s.kf(0, 2, stereo=True, close=[0, 1])
    _observers(s, 1, 3, 2, stereo=True)
    for p in (0, 1):
        for k in range(4):
            s.see(p, k, p)
    return dict(name=name, scene=s, local=[0], not_erase=[0], monocular=mono, expect=expect)


def _boundary(n, name, expect):
    # keyframe 0 has n points; all but the last are seen by keyframes 1-3 as well, the last by keyframe 1 only
    s = Scene()
    s.kf(0, n)
    _observers(s, 1, 3, n)
    for p in range(n):
        s.see(p, 0, p)
        for k in (1, 2, 3) if p < n - 1 else (1,):
            s.see(p, k, p)
    return dict(name=name, scene=s, local=[0], not_erase=[0], monocular=True, expect=expect)


def _not_erase():
    # keyframes 0-3 all see points 0-4.  0 is redundant but mbNotErase; 1 is redundant only because 0 still counts as an observer
    s = Scene()
    _observers(s, 0, 4, 5)
    for p in range(5):
        for k in range(4):
            s.see(p, k, p)
    return dict(name="not_erase", scene=s, local=[0, 1], not_erase=[1, 0], monocular=True,
                expect=dict(culled=[2, 1], n_mps=[5, 5], n_redundant=[5, 5], bad_points=[]))


def _cascade_a():
    # keyframes 0-3 all see points 0-5: 0 and 1 are each redundant only while the other lives (nObs 4 -> 3 once 0 is gone)
    s = Scene()
    _observers(s, 0, 4, 6)
    for p in range(6):
        for k in range(4):
            s.see(p, k, p)
    return dict(name="cascade_a", scene=s, local=[0, 1], not_erase=[0, 0], monocular=True,
                expect=dict(culled=[1, 0], n_mps=[6, 6], n_redundant=[6, 0], bad_points=[]))


def _cascade_b():
    # keyframe 0: points 0-10 redundant (seen by 2, 3, 4 too) and point 20 at a stereo feature (weight 2), which 5 and 6 see mono: nObs 4.
    # keyframe 1: points 100-108 redundant (seen by 2, 3, 4), point 109 seen by 2 only, and a match to point 20 without an observation:
    # 10 of 11 on the untouched graph, culled.  Culling 0 takes point 20 to nObs 2: bad; it leaves nMPs and nRedundant of 1: 9 of 10, kept.
    s = Scene()
    s.kf(0, 12, stereo=[0] * 11 + [1])
    s.kf(1, 11)
    _observers(s, 2, 3, 24)
    _observers(s, 5, 2, 1)
    for p in range(11):
        s.see(p, 0, p)
        for k in (2, 3, 4):
            s.see(p, k, p)
    s.see(20, 0, 11); s.see(20, 5, 0); s.see(20, 6, 0)
    for j in range(10):
        s.see(100 + j, 1, j)
        for k in (2, 3, 4) if j < 9 else (2,):
            s.see(100 + j, k, 12 + j)
    s.match(1, 10, 20)
    return dict(name="cascade_b", scene=s, local=[0, 1], not_erase=[0, 0], monocular=True,
                expect=dict(culled=[1, 0], n_mps=[12, 10], n_redundant=[11, 9], bad_points=[20]), alone={1: (1, 11, 10)})


CULL_CASES = [
    _scale((3, 3, 3), "scale_plus_one_counts", dict(culled=[1], n_mps=[1], n_redundant=[1], bad_points=[])),
    _scale((3, 3, 4), "scale_plus_two_does_not", dict(culled=[0], n_mps=[1], n_redundant=[0], bad_points=[])),
    _scale((0, 1, 2), "finer_scales_count", dict(culled=[1], n_mps=[1], n_redundant=[1], bad_points=[])),
    _nobs((2, 2), "two_observers_not_redundant", dict(culled=[0], n_mps=[1], n_redundant=[0], bad_points=[]), own=2),   # nObs 6, 2 others
    _nobs((1, 1, 1), "nobs_3_does_not_qualify", dict(culled=[0], n_mps=[1], n_redundant=[0], bad_points=[])),       # 3 others, nObs 3
    _nobs((2, 1, 1), "nobs_4_qualifies", dict(culled=[1], n_mps=[1], n_redundant=[1], bad_points=[])),              # 3 others, nObs 4
    _nobs((2,), "nobs_4_two_stereo_observations", dict(culled=[0], n_mps=[1], n_redundant=[0], bad_points=[]), own=2),  # scanned: 1 other
    _far(False, "far_skipped_in_stereo", dict(culled=[1], n_mps=[1], n_redundant=[1], bad_points=[])),
    _far(True, "far_counted_monocular", dict(culled=[1], n_mps=[2], n_redundant=[2], bad_points=[])),
    _boundary(10, "nine_of_ten_kept", dict(culled=[0], n_mps=[10], n_redundant=[9], bad_points=[])),
    _boundary(11, "ten_of_eleven_culled", dict(culled=[1], n_mps=[11], n_redundant=[10], bad_points=[10])),
    _not_erase(),
    _cascade_a(),
    _cascade_b(),
]


def random_cull_scene(seed):
    """-> (scene, local, not_erase, monocular): at most 12 local keyframes x 64 features, a few more keyframes that only observe.
    Points are seen by 2-6 keyframes drawn from a window of neighbours, so that some keyframes are redundant, some are redundant only
    through one another, and some points sit at nObs 3-4 where one cull takes them to bad."""
    r = np.random.RandomState(seed)
    n_local = int(r.randint(2, 13))
    n_kf = n_local + int(r.randint(0, 4))
    nfeat = [int(r.randint(8, 65)) for _ in range(n_kf)]
    mono = bool(r.randint(0, 2))
    p_stereo = 0.0 if mono else 0.7
    spread = r.rand() < 0.4                  # octaves 0-3, so that the scale rule decides; otherwise 1-2, where every observer counts
    s = Scene()
    for k in range(n_kf):
        st = r.rand(nfeat[k]) < p_stereo
        s.kf(k, nfeat[k], octave=r.randint(0, 4, nfeat[k]) if spread else r.randint(1, 3, nfeat[k]), stereo=st,
             close=(r.rand(nfeat[k]) < 0.85) & st if not mono else [1] * nfeat[k])
    free = [list(r.permutation(nfeat[k])) for k in range(n_kf)]
    dense = r.choice([2, 3, 4, 5, 6], p=[0.05, 0.1, 0.35, 0.3, 0.2])      # the typical number of observers in this scene
    weak = r.choice([0.0, 0.04, 0.08])                                      # the share of points with two or three observers whatever `dense`
    p = 0
    for _ in range(int(sum(nfeat) / dense * r.uniform(0.6, 1.0))):
        m = int(r.randint(2, 4)) if r.rand() < weak else int(np.clip(dense + r.randint(-1, 2), 2, min(6, n_kf)))
        c = int(r.randint(0, n_kf))
        win = [k for k in range(c - 4, c + 5) if 0 <= k < n_kf and free[k]]
        if len(win) < 2:
            continue
        ks = r.choice(win, min(m, len(win)), replace=False)
        for j, k in enumerate(ks):
            i = int(free[int(k)].pop())
            u = r.rand()
            if j == 0 or u < 0.92:         # the first keyframe always in both views: a point exists from its first observation on
                s.see(p, int(k), i)
            elif u < 0.96:
                s.match(int(k), i, p)      # a match without an observation
            else:
                s.obs(p, int(k), i)        # an observation without a match
        p += 1
    local = [int(k) for k in r.permutation(n_kf)[:n_local]]
    not_erase = [int(r.rand() < 0.1) for _ in local]
    return s, local, not_erase, mono
