"""Seeded scenes for the PoseOptimization tests: points 2-30 units in front of a camera with KITTI-like intrinsics, pixel noise drawn per
pyramid level, gross outliers, one finite point behind the camera, features without a point interleaved, and a start pose a few degrees
and a few percent of the depth away from the truth."""
import math

import numpy as np

f32 = np.float32
CAM = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448], f32)     # fx fy cx cy mbf (KITTI 00-02)
W, H = 1241.0, 376.0
NLEVELS = 8
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(NLEVELS)], np.float64)
INV_SIGMA2 = (1.0 / SIGMA2).astype(f32)                                   # mvInvLevelSigma2

SIZES = (0, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 1000)
MIXES = ("mono", "stereo", "mixed")


def rodrigues(r):
    th = float(np.linalg.norm(r))
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def scene(seed, n_corr, mix="mixed", outlier_frac=0.3, behind=True, noise=True, spare=None, perturb=1.0):
    """-> dict(obs=dict(x, y, u_right, inv_sigma2, Xw, has_point), octave, cam, Tcw (float32 start pose), Tcw_true (double), gross (bool
    per feature: made a gross outlier or put behind the camera))"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = n_corr + (n_corr // 2 + 3 if spare is None else spare)
    has = np.zeros(n, np.uint8)
    has[np.sort(rng.permutation(n)[:n_corr])] = 1
    R = rodrigues(rng.normal(0, 0.2, 3))
    t = rng.normal(0, 2.0, 3)
    u = rng.uniform(20, W - 20, n); v = rng.uniform(20, H - 20, n); z = rng.uniform(2.0, 30.0, n)
    fx, fy, cx, cy, bf = [float(c) for c in CAM]
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    gross = np.zeros(n, bool)
    i_behind = -1
    if behind and n_corr >= 10:
        i_behind = int(np.nonzero(has)[0][n_corr // 2])
        Pc[i_behind] = [1.0, 0.5, -5.0]
        gross[i_behind] = True
    Xw = ((Pc - t) @ R).astype(f32)                                        # R^T (Pc - t)
    Pt = Xw.astype(np.float64) @ R.T + t
    octave = rng.integers(0, NLEVELS, n).astype(np.int32)
    sig = np.sqrt(SIGMA2[octave]) * (1.0 if noise else 0.0)
    x = Pt[:, 0] / Pt[:, 2] * fx + cx + rng.normal(0, 1, n) * sig
    y = Pt[:, 1] / Pt[:, 2] * fy + cy + rng.normal(0, 1, n) * sig
    ur = Pt[:, 0] / Pt[:, 2] * fx + cx - bf / Pt[:, 2] + rng.normal(0, 1, n) * sig
    if i_behind >= 0:   # the reference has no depth test here: the point projects mirrored, and only a measurement elsewhere makes it an outlier
        x[i_behind] += 150.0; y[i_behind] += 80.0; ur[i_behind] = x[i_behind] - 40.0
    pick = rng.random(n) < outlier_frac
    pick &= ~gross
    off = rng.uniform(20, 100, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    x = np.where(pick, x + off[:, 0], x); y = np.where(pick, y + off[:, 1], y); ur = np.where(pick, ur + off[:, 2], ur)
    gross |= pick
    if mix == "mono":
        stereo = np.zeros(n, bool)
    elif mix == "stereo":
        stereo = np.ones(n, bool)
    else:
        stereo = rng.random(n) < 0.5
    ur = np.where(stereo, np.maximum(ur, 0.0), -1.0)                      # mvuRight: -1 where no stereo match
    # the start pose: a few degrees, a few percent of the depth
    dR = rodrigues(rng.normal(0, math.radians(1.5), 3) * perturb)
    dt = rng.normal(0, 0.15, 3) * perturb
    T0 = np.eye(4)
    T0[:3, :3] = dR @ R
    T0[:3, 3] = dR @ t + dt
    Tt = np.eye(4); Tt[:3, :3] = R; Tt[:3, 3] = t
    Tcw = T0.astype(f32)
    z0 = (Xw.astype(np.float64) @ Tcw[:3, :3].astype(np.float64).T + Tcw[:3, 3].astype(np.float64))[:, 2]
    ok = (z0 > 0.1) | (Pc[:, 2] < 0)
    assert ok.all(), "a point too close to the camera at the start pose"
    obs = dict(x=x.astype(f32), y=y.astype(f32), u_right=ur.astype(f32), inv_sigma2=INV_SIGMA2[octave], Xw=Xw, has_point=has)
    return dict(obs=obs, octave=octave, cam=CAM, Tcw=Tcw, Tcw_true=Tt, gross=gross & has.astype(bool), stereo=stereo)


def admissible(n_corr, sc, results):
    """The condition on a test scene, on the model alone (results: tests/pose_model.py's optimize() in its three summation orders):
    the orders agree on every discrete result and took the same accept / reject path through the Levenberg loops (a scene on which
    rounding of the size the orders differ by turns a decision is one on which a fourth summation order, the GPU's, may turn it too);
    no edge of any round within 1e-6 of its threshold and no evaluation of the stop rule within 1e-6 of its limit; and with 10 or more
    correspondences all four rounds run, they reclassify, and every gross outlier (the point behind the camera among them) ends as one."""
    import pose_model as pm
    a = results[0]
    if not all(r["rounds"] == a["rounds"] and r["n_bad"] == a["n_bad"] and (r["outlier"] == a["outlier"]).all() for r in results[1:]):
        return False
    if not pm.same_path(results):
        return False
    for r in results:
        if min([float(m.min()) for m in r["margin"] if len(m)] or [1.0]) < 1e-6 or pm.path_sensitivity(r)[1] < 1e-6:
            return False
    if n_corr >= 10 and (a["rounds"] != 4 or len(set(a["n_bad"])) < 2 or not a["outlier"][sc["gross"]].all()):
        return False
    return True


def seed_of(n_corr, mix):
    """the seeds of the GPU tests: the first of base, base + 5000, base + 10000, ... whose scene is admissible (tools/pose_spread.py --select
    finds the shifts; tests/test_pose_model.py checks every one of them on the CPU)"""
    return 1000 * MIXES.index(mix) + n_corr + 5000 * SEED_SHIFT.get((n_corr, mix), 0)


SEED_SHIFT = {(3, 'mono'): 2, (10, 'mono'): 6, (10, 'mixed'): 5, (63, 'stereo'): 1, (63, 'mixed'): 3, (64, 'mono'): 9, (64, 'stereo'): 6,
              (65, 'mono'): 23, (255, 'mono'): 9, (255, 'stereo'): 3, (256, 'mono'): 2, (256, 'stereo'): 1, (257, 'mono'): 12,
              (1000, 'mono'): 7}


def all_scenes():
    return [(n, mix, scene(seed_of(n, mix), n, mix)) for n in SIZES for mix in MIXES]
