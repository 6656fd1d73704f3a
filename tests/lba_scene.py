"""Seeded scenes for the local bundle adjustment tests: keyframes on an arc looking at a point cloud, every point seen by 2-6 of them,
pixel noise, 10 % gross outliers, one point behind a camera, float start values perturbed from the truth.

SHAPES are (free, fixed, points), the smallest that cross each structural boundary: one row, a few rows, 6K past 64 (11 free keyframes)
and past 256 (43).  MIXES: "mono", "stereo", "mixed"; a monocular scene always holds at least two fixed keyframes (the scale gauge).
SPECIAL names the scenes that produce one case each (the last two are the ones in which computeLambdaInit is decided by a point's
diagonal: no other scene can tell a maximum over all vertices from one over the poses).  scene(...) -> dict(problem=..., truth_pose [K][3][4], truth_X, gross [E] bool,
behind [E] bool, and what a special scene plants).  admissible(scene, results): the condition every scene must satisfy on the model."""
import math

import numpy as np

f32 = np.float32
SHAPES = [(1, 1, 8), (2, 2, 20), (3, 2, 64), (11, 3, 200), (22, 5, 400), (43, 6, 600)]
MIXES = ("mono", "stereo", "mixed")
SPECIAL = ("point_all_level1", "kf_all_level1", "single_edge", "fixed_only_point", "fixed_in_middle", "no_edges", "no_points", "few_edges_near",
           "all_fixed")
FX, FY, CX, CY, BF = 500.0, 500.0, 320.0, 240.0, 40.0
NLEVELS = 4
MARGIN = 1e-6
# tools/lba_spread.py --select: the first seed shift per (shape, mix) whose scene is admissible (absent: 0)
SEED_SHIFT = {((1, 1, 8), 'mixed'): 2, ((22, 5, 400), 'mixed'): 1}
SPECIAL_SHIFT = {'fixed_only_point': 1, 'few_edges_near': 2}
DROPPED = set()   # (shape, mix) without an admissible seed among 32 shifts


def seed_of(shape, mix):
    return 100 * SHAPES.index(shape) + 10 * MIXES.index(mix) + 7 + 5000 * SEED_SHIFT.get((shape, mix), 0)


def _look_at(centre, target):
    """world -> camera [R | t] of a camera at `centre` whose z axis points at `target`, y down"""
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ centre


def _rodrigues(v):
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def _project(R, t, X, stereo):
    Pc = R @ X + t
    u = FX * Pc[0] / Pc[2] + CX
    v = FY * Pc[1] / Pc[2] + CY
    return u, v, (u - BF / Pc[2]) if stereo else -1.0, Pc[2]


def scene(seed, free, fixed, points, mix, noise=0.5, outliers=0.1, behind=True, special=None, perturb=1.0, max_views=6, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    if mix == "mono":
        fixed = max(fixed, 2)
    K = free + fixed
    ang = np.linspace(-0.7, 0.7, K) if K > 1 else np.zeros(1)
    Rs, ts = [], []
    for a in ang:
        c = scale * (np.array([4.0 * math.sin(a), rng.uniform(-0.3, 0.3), -4.0 * math.cos(a)]) + rng.uniform(-0.1, 0.1, 3))
        R, t = _look_at(c, scale * rng.uniform(-0.2, 0.2, 3))
        Rs.append(R); ts.append(t)
    is_fixed = np.zeros(K, np.uint8)
    is_fixed[free:] = 1                                                  # the local keyframes first, lFixedCameras behind them
    if special == "fixed_in_middle":                                     # the keyframe with mnId == 0 among the local ones
        is_fixed[:] = 0
        is_fixed[free // 2] = 1
        is_fixed[K - (fixed - 1):] = 1 if fixed > 1 else 0
    X = scale * rng.normal(0.0, 0.6, (points, 3))
    kf_stereo = np.array([mix == "stereo" or (mix == "mixed" and k % 2 == 0) for k in range(K)])
    if special == "no_points":
        X = X[:0]
    ek, ep, mx, my, mr, isig, gross, bh = [], [], [], [], [], [], [], []
    plant = {}
    P = len(X)
    p_behind = P - 1 if (behind and P > 2) else -1
    sp_point = 0 if special in ("point_all_level1", "single_edge", "fixed_only_point") else -1
    sp_kf = 0 if special == "kf_all_level1" else -1
    free_ids, fixed_ids = np.nonzero(is_fixed == 0)[0], np.nonzero(is_fixed)[0]
    for p in range(P):
        nv = int(rng.integers(2, min(max_views, K) + 1))
        seen = rng.permutation(K)[:nv]
        if sp_kf >= 0:
            seen = seen[seen != sp_kf]
            if p < 8:
                seen = np.concatenate([seen, [sp_kf]])                   # the special keyframe sees eight points only, each at a wrong place
            if len(seen) < 2:
                seen = np.array([k for k in range(K) if k != sp_kf][:2])
        if special == "few_edges_near":                                  # the one free keyframe sees the first three points only
            seen = seen[seen != 0]
            if p < 3:
                seen = np.concatenate([seen, [0]])
            if len(seen) < 2:
                seen = np.array(list(seen) + [k for k in range(1, K) if k not in seen][:2 - len(seen)])
        if special == "single_edge" and p == sp_point:
            seen = np.array([k for k in free_ids if kf_stereo[k]][:1])   # a stereo edge: a single monocular edge leaves Hll singular
        if special == "fixed_only_point" and p == sp_point:
            seen = fixed_ids[:2]
        if p == p_behind:                                                # beyond keyframe 0's centre, along its backward axis
            c0 = -Rs[0].T @ ts[0]
            X[p] = c0 + scale * (-1.5 * Rs[0][2] + rng.uniform(-0.05, 0.05, 3))
            far = [k for k in range(1, K) if (Rs[k] @ X[p] + ts[k])[2] > 2.0 * scale and k != sp_kf]      # in front of these, well away from z = 0
            seen = np.array([0] + far[-3:])
        seen = rng.permutation(seen) if special != "kf_all_level1" else seen
        n_gross = 0
        for k in seen:
            u, v, r, z = _project(Rs[k], ts[k], X[p], kf_stereo[k])
            octave = int(rng.integers(0, NLEVELS))
            sig = 1.2 ** octave
            is_behind = z <= 0
            # a gross outlier only where three good views of the point remain: a point that round 2 leaves with one monocular edge has a
            # singular Hll, and its 1 / lambda would set the scene's condition
            g = (not is_behind) and p != p_behind and rng.uniform() < 2.0 * outliers and n_gross < len(seen) - 3
            n_gross += g
            if (special == "point_all_level1" and p == sp_point) or (sp_kf >= 0 and k == sp_kf):
                g = True
            du, dv = rng.normal(0, noise * sig, 2) if noise > 0 else (0.0, 0.0)
            if g:
                off = rng.uniform(25.0, 60.0, 2) * rng.choice([-1.0, 1.0], 2)
                du, dv = du + off[0], dv + off[1]
            ek.append(k); ep.append(p); mx.append(u + du); my.append(v + dv)
            mr.append(r + du + (rng.normal(0, noise * sig) if noise > 0 else 0.0) if kf_stereo[k] else -1.0)
            isig.append(1.0 / (sig * sig)); gross.append(g); bh.append(is_behind)
    if special == "no_edges":
        ek, ep, mx, my, mr, isig, gross, bh = [], [], [], [], [], [], [], []
    # the start values: the truth, the free keyframes and the points perturbed, everything cast to float
    Tcw = np.zeros((K, 4, 4), f32)
    truth = np.zeros((K, 3, 4))
    for k in range(K):
        R, t = Rs[k], ts[k]
        truth[k, :, :3], truth[k, :, 3] = R, t
        if not is_fixed[k]:
            R = _rodrigues(rng.normal(0, 0.01 * perturb, 3)) @ R
            t = t + scale * rng.normal(0, 0.02 * perturb, 3)
        Tcw[k, :3, :3], Tcw[k, :3, 3], Tcw[k, 3, 3] = R, t, 1.0
    Xw = (X + scale * rng.normal(0, 0.02 * perturb, X.shape)).astype(f32)
    cam = np.tile(np.array([FX, FY, CX, CY, BF], f32), (K, 1))
    problem = dict(Tcw=Tcw, cam=cam, fixed=is_fixed, Xw=Xw, edge_kf=np.array(ek, np.int32), edge_point=np.array(ep, np.int32),
                   x=np.array(mx, f32), y=np.array(my, f32), u_right=np.array(mr, f32), inv_sigma2=np.array(isig, f32))
    plant.update(sp_point=sp_point, sp_kf=sp_kf, p_behind=p_behind)
    return dict(problem=problem, truth_pose=truth, truth_X=X, gross=np.array(gross, bool), behind=np.array(bh, bool), plant=plant,
                special=special, mix=mix)


def shape_scene(shape, mix, shift=None):
    seed = seed_of(shape, mix) if shift is None else 100 * SHAPES.index(shape) + 10 * MIXES.index(mix) + 7 + 5000 * shift
    return scene(seed, shape[0], shape[1], shape[2], mix)


def special_scene(name, shift=None):
    shift = SPECIAL_SHIFT.get(name, 0) if shift is None else shift
    seed = 900 + SPECIAL.index(name) + 5000 * shift
    if name == "few_edges_near":     # a free keyframe with three edges, six fixed ones with many, depths about 0.4 (a monocular map normalised to a
        # median depth of 1 has such depths): a point's Hll diagonal exceeds every Hpp diagonal, so lambdaInit is decided by the POINTS
        return scene(seed, 1, 6, 12, "stereo", outliers=0.0, behind=False, special=name, max_views=7, scale=0.1)
    if name == "all_fixed":          # no free keyframe: no row, no reduced system, the points alone are optimised and alone decide lambdaInit
        return scene(seed, 0, 5, 64, "mixed", special=name)
    return scene(seed, 3, 2, 64, "mixed", special=name)


def all_scenes():
    """-> (tag, scene) of every scene of the tests"""
    for shape in SHAPES:
        for mix in MIXES:
            if (shape, mix) not in DROPPED:
                yield f"{shape[0]}-{shape[1]}-{shape[2]}-{mix}", shape_scene(shape, mix)
    for name in SPECIAL:
        yield name, special_scene(name)


def admissible(sc, results):
    """the model's three summation orders agree on every flag, count and accept / reject path; no edge lies within MARGIN of its chi2
    threshold and no depth within MARGIN of zero, at either classification"""
    a = results[0]
    for r in results:
        if not (r["margin_chi2"] >= MARGIN and r["margin_depth"] >= MARGIN):
            return False
        if r["edge_flags"].tobytes() != a["edge_flags"].tobytes() or r["decisions"] != a["decisions"]:
            return False
        for k in ("stopped", "iterations", "trials", "n_level1", "n_erase", "n_active_kf", "n_active_points"):
            if r[k] != a[k]:
                return False
        if not (np.isfinite(r["pose"]).all() and np.isfinite(r["point"]).all()):
            return False
    return True
