"""Small maps for the tests of orbx_mapgraph_refresh_points: keyframes with camera centres, octaves and descriptors, points with positions,
reference keyframes and rows.  A scene is applied through the calls that mapgraph_model.SlotGraph and orbx.MapGraph share, so one scene
drives the model and the device; `order` changes only the order in which the rows are written."""
import numpy as np

from mapgraph_model import SlotGraph
import refresh_model as rm

SCALE_FACTORS = np.array([1.2 ** l for l in range(8)], np.float32)
PATTERN = 0xA5


class Scene:
    def __init__(self, seed, n_kf, n_feat, n_pts, max_obs, rows=None, max_row=None):
        r = np.random.RandomState(seed)
        self.limits = (n_kf, n_feat, n_pts, max_obs)
        self.n_kf, self.n_feat, self.n_pts = n_kf, n_feat, n_pts
        self.centre = (r.rand(n_kf, 3).astype(np.float32) - np.float32(0.5)) * np.float32(4.0)
        self.centre[:, 2] -= np.float32(6.0)
        self.octave = r.randint(0, 8, (n_kf, n_feat)).astype(np.uint8)
        self.desc = r.randint(0, 256, (n_kf, n_feat, 32)).astype(np.uint8)
        self.xy = (r.rand(n_kf, n_feat, 2) * np.array([630.0, 470.0]) + 5.0).astype(np.float32)
        self.pos = (r.rand(n_pts, 3).astype(np.float32) - np.float32(0.5)) * np.float32(3.0)
        if rows is None:
            rows = {}
            top = min(n_kf, max_obs) if max_row is None else max_row
            for p in range(n_pts):
                ks = r.permutation(n_kf)[:r.randint(1, top + 1)]
                rows[p] = [(int(k), int(r.randint(0, n_feat))) for k in ks]
        self.rows = rows
        self.ref_kf = np.array([rows[p][r.randint(0, len(rows[p]))][0] if p in rows else 0 for p in range(n_pts)], np.int32)
        # matches: most follow the observations, some name another point or none (the two views may disagree)
        self.matches = {}
        for p, row in rows.items():
            for k, i in row:
                u = r.rand()
                self.matches[(k, i)] = p if u < 0.8 else (int(r.randint(0, n_pts)) if u < 0.9 else -1)
        self.rng = r

    def frame(self, k):
        n = self.n_feat
        return dict(x=self.xy[k, :, 0], y=self.xy[k, :, 1], octave=self.octave[k].astype(np.int32), angle=np.zeros(n, np.float32),
                    u_right=np.full(n, -1, np.float32), desc=self.desc[k], bounds=(0.0, 0.0, 640.0, 480.0))

    def apply(self, target, order="forward", extras=False):
        """the scene through the edit calls of `target`.  extras: every row of three or more first gets observers it does not keep, which
        are erased again -- the last entry moves into each gap, so the stored order is shuffled once more"""
        zero = np.zeros(self.n_feat, np.uint8)
        for k in range(self.n_kf):
            target.set_keyframe(k, self.octave[k], zero, zero)
        obs = [(p, k, i) for p, row in sorted(self.rows.items()) for k, i in row]
        if order == "reversed":
            obs = obs[::-1]
        elif order == "shuffled":
            obs = [obs[j] for j in np.random.RandomState(99).permutation(len(obs))]
        extra = []
        if extras:
            for p, row in sorted(self.rows.items()):
                free = [k for k in range(self.n_kf) if k not in {k for k, _ in row}]
                if len(row) >= 3 and len(row) < self.limits[3] and free:
                    extra.append((p, free[0], 0))
            if extra:
                target.add_observations(*zip(*extra))
        target.add_observations(*zip(*obs))
        if extra:
            target.erase_observations([e[0] for e in extra], [e[1] for e in extra])
        by_kf = {}
        for (k, i), p in sorted(self.matches.items()):
            by_kf.setdefault(k, []).append((i, p))
        for k, lst in by_kf.items():
            target.set_matches(k, [a for a, _ in lst], [b for _, b in lst])

    def model(self):
        sg = SlotGraph(*self.limits)
        self.apply(sg)
        return sg

    def keyframes(self, frames=None, bad=(), slots=None):
        """the keyframe table of a job: every slot (or `slots`), shuffled so that the list's order differs from the slots'"""
        ks = list(range(self.n_kf)) if slots is None else list(slots)
        ks = [ks[j] for j in np.random.RandomState(7).permutation(len(ks))]
        return dict(slot=np.array(ks, np.int32), centre=self.centre[ks], bad=np.array([1 if k in bad else 0 for k in ks], np.uint8),
                    frame=[None if frames is None else frames[k] for k in ks])

    def expect(self, sg, points, what, bad=(), pos=None, ref_kf=None, centre=None, scale_factors=SCALE_FACTORS):
        pos = self.pos if pos is None else pos
        ref = self.ref_kf if ref_kf is None else ref_kf
        cen = self.centre if centre is None else centre
        return rm.refresh(sg, points, what, pos=[pos[p] for p in points], ref_kf=[ref[p] for p in points],
                          centre={k: cen[k] for k in range(self.n_kf)}, bad={k: k in bad for k in range(self.n_kf)},
                          frame_desc={k: self.desc[k] for k in range(self.n_kf)}, scale_factors=scale_factors)
