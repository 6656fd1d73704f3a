"""Seeded scenes for the OptimizeSim3 tests: two keyframes that see the same points through maps related by a Sim3 (a loop candidate: the
second map has drifted), pixel noise drawn per pyramid level, gross outliers, features without a pair interleaved, and a start estimate a
few degrees and a few percent away from the truth.  The camera-frame points are formed as the reference forms them (src/Optimizer.cc:
1241-1251), from float world points and float keyframe poses by the cv::Mat rule: camera_points() below, which the package's
sim3opt_camera_points has to reproduce bit for bit."""
import math

import numpy as np

from pose_scene import INV_SIGMA2, NLEVELS, SIGMA2, rodrigues

f32 = np.float32
CAM1 = np.array([718.856, 718.856, 607.1928, 185.2157], f32)              # fx fy cx cy (KITTI 00-02)
CAM2 = np.array([707.0912, 707.0912, 601.8873, 183.1104], f32)            # (KITTI 04-12): the two cameras differ, so a swap shows
W, H = 1241.0, 376.0
TH2 = 10.0                                                                # LoopClosing::ComputeSim3: OptimizeSim3(..., 10, mbFixScale)

N_CORR = (0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257)
KINDS = ("clean", "outliers", "starved")
# clean: no gross outlier (round 2 runs 5 iterations); outliers: about a fifth of the pairs are gross outliers (10 iterations);
# starved: so many that fewer than 10 pairs are left after round 1 (return 0, g2oS12 untouched, the flags of round 1 cleared)


def camera_points(Xw, Rcw, tcw):
    """(float)(double products, double sum) then the float add of t: `Rcw * Xw + tcw` on CV_32F matrices"""
    X = np.asarray(Xw, f32).astype(np.float64)
    R = np.asarray(Rcw, f32).astype(np.float64)
    P = np.stack([((X[:, 0] * R[r, 0] + X[:, 1] * R[r, 1]) + X[:, 2] * R[r, 2]).astype(f32) for r in range(3)], axis=1)
    return P + np.asarray(tcw, f32)[None, :]


def quat_of(R):
    """a unit quaternion (x, y, z, w) of a rotation matrix, w >= 0"""
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def scene(seed, n_corr, kind="outliers", fix_scale=False, unit_start=False):
    """-> dict(obs=dict(has_pair, P1c, P2c, x1, y1, inv_sigma2_1, x2, y2, inv_sigma2_2), cam1, cam2, S12 (the start, 8 doubles), S12_true,
    th2, fix_scale, gross (bool per feature), world=dict(Xw1, R1w, t1w, Xw2, R2w, t2w): what P1c and P2c were formed from).
    fix_scale scenes have a true scale of 1 (stereo / RGB-D); unit_start makes the start's scale exactly 1 where the truth is not."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = n_corr + n_corr // 2 + 3
    has = np.zeros(n, np.uint8)
    has[np.sort(rng.permutation(n)[:n_corr])] = 1
    # the truth: P1c = s R P2c + t
    s_true = 1.0 if fix_scale else float(rng.uniform(1.15, 1.35))
    R_true = rodrigues(rng.normal(0, 0.12, 3))
    t_true = rng.normal(0, 0.6, 3)
    f2 = [float(c) for c in CAM2]
    f1 = [float(c) for c in CAM1]
    P2, tries = np.zeros((0, 3)), 0
    while len(P2) < n:                                                    # points both cameras see, 3 - 30 units away
        u = rng.uniform(20, W - 20, 4 * n + 16); v = rng.uniform(20, H - 20, 4 * n + 16); z = rng.uniform(3.0, 30.0, 4 * n + 16)
        c = np.stack([(u - f2[2]) / f2[0] * z, (v - f2[3]) / f2[1] * z, z], axis=1)
        p1 = s_true * c @ R_true.T + t_true
        ok = (p1[:, 2] > 2.0) & (np.abs(p1[:, 0] / p1[:, 2] * f1[0] + f1[2] - W / 2) < W / 2 + 300) & \
            (np.abs(p1[:, 1] / p1[:, 2] * f1[1] + f1[3] - H / 2) < H / 2 + 300)
        P2 = np.concatenate([P2, c[ok]])[:n]
        tries += 1
        assert tries < 50
    # the two keyframes and their maps: Xw = Rcw^T (Pc - tcw), float; the camera-frame points come back through camera_points
    world = {}
    Pc = {}
    for k, P in ((1, s_true * P2 @ R_true.T + t_true), (2, P2)):
        Rw = rodrigues(rng.normal(0, 0.3, 3)).astype(f32)
        tw = rng.normal(0, 3.0, 3).astype(f32)
        Xw = ((P - tw.astype(np.float64)) @ Rw.astype(np.float64)).astype(f32)
        world[f"Xw{k}"], world[f"R{k}w"], world[f"t{k}w"] = Xw, Rw, tw
        Pc[k] = camera_points(Xw, Rw, tw)
    P1c, P2c = Pc[1], Pc[2]
    oct1 = rng.integers(0, NLEVELS, n); oct2 = rng.integers(0, NLEVELS, n)
    sig = 0.5 if kind == "clean" else 0.8                                 # of the level's sigma: a clean scene has no pair near th2
    d1, d2 = P1c.astype(np.float64), P2c.astype(np.float64)
    x1 = d1[:, 0] / d1[:, 2] * f1[0] + f1[2] + rng.normal(0, sig, n) * np.sqrt(SIGMA2[oct1])
    y1 = d1[:, 1] / d1[:, 2] * f1[1] + f1[3] + rng.normal(0, sig, n) * np.sqrt(SIGMA2[oct1])
    x2 = d2[:, 0] / d2[:, 2] * f2[0] + f2[2] + rng.normal(0, sig, n) * np.sqrt(SIGMA2[oct2])
    y2 = d2[:, 1] / d2[:, 2] * f2[1] + f2[3] + rng.normal(0, sig, n) * np.sqrt(SIGMA2[oct2])
    gross = np.zeros(n, bool)
    pairs = np.nonzero(has)[0]
    if kind == "outliers":                                                # about a fifth, but round 2 stays reachable from 11 pairs on
        k = max(1, int(round(0.2 * n_corr)))
        if n_corr >= 11:
            k = min(k, n_corr - 10)
        gross[rng.permutation(pairs)[:k]] = True
    elif kind == "starved":                                               # at most 6 good pairs
        gross[rng.permutation(pairs)[6:]] = True
    off = rng.uniform(25, 120, (n, 4)) * rng.choice([-1.0, 1.0], (n, 4))
    side = rng.random(n) < 0.5                                            # a gross outlier is wrong in one image or the other
    x1 = np.where(gross & side, x1 + off[:, 0], x1); y1 = np.where(gross & side, y1 + off[:, 1], y1)
    x2 = np.where(gross & ~side, x2 + off[:, 2], x2); y2 = np.where(gross & ~side, y2 + off[:, 3], y2)
    # the start: a few degrees and a few percent off
    dR = rodrigues(rng.normal(0, math.radians(1.5), 3))
    q0 = quat_of(dR @ R_true)
    t0 = dR @ t_true + rng.normal(0, 0.05, 3)
    s0 = 1.0 if (fix_scale or unit_start) else s_true * float(1.0 + rng.normal(0, 0.03))
    obs = dict(has_pair=has, P1c=P1c, P2c=P2c, x1=x1.astype(f32), y1=y1.astype(f32), inv_sigma2_1=INV_SIGMA2[oct1],
               x2=x2.astype(f32), y2=y2.astype(f32), inv_sigma2_2=INV_SIGMA2[oct2])
    return dict(obs=obs, cam1=CAM1, cam2=CAM2, S12=np.concatenate([q0, t0, [s0]]), S12_true=np.concatenate([quat_of(R_true), t_true, [s_true]]),
                th2=TH2, fix_scale=bool(fix_scale), gross=gross & has.astype(bool), world=world, kind=kind)


def args(sc):
    return sc["obs"], sc["cam1"], sc["cam2"], sc["S12"], sc["th2"], sc["fix_scale"]


# ---------------------------------------------------------------- the scenes of the tests

VARIANTS = (dict(order="asc"), dict(order="desc"), dict(order="pair"), dict(nudge=1), dict(nudge=2), dict(jacobian="closed"))
NOISE_STEP = 1e-8     # the variants have to agree on every damping trial that moves the estimate by this much or more


def case_flags(n_corr, kind):
    """fix_scale and unit_start of a case: both values of each, spread over the sizes and kinds"""
    k = N_CORR.index(n_corr) + KINDS.index(kind)
    return bool(k & 1), bool(k & 2)


def expected_exit(n_corr, kind):
    """-> (rounds, more_iterations or None, returns a count) the case is built to reach"""
    if n_corr == 0:
        return 0, 5, False
    if n_corr < 10 or kind == "starved" or (kind == "outliers" and n_corr == 10):
        return 1, (None if kind == "starved" and n_corr <= 6 else 5 if kind == "clean" else 10), False
    return 2, (5 if kind == "clean" else 10), True


def variants(sc):
    """the model's answer in every variant (tests/sim3opt_model.py), the plain one first"""
    import sim3opt_model as sm
    return [sm.optimize(*args(sc), **v) for v in sc.get("variants", VARIANTS)]


def firm_decisions(res):
    """the accept / reject decisions on trials that move the estimate by NOISE_STEP or more (max |x_j|), as (round, accepted)"""
    return [(rnd, accepted) for (rnd, _, _, accepted, _, _, xmax) in res["decisions"] if xmax >= NOISE_STEP]


def class_spread(results):
    """the largest disagreement of the variants on the chi2 of an edge at a classification, and the smallest distance of such a chi2
    from th2 (both absolute); (0, inf) where nothing was classified"""
    a = results[0]
    spread, margin = 0.0, math.inf
    for k in range(a["rounds"]):
        for r in results:
            if len(r["class_chi2"]) <= k or r["class_chi2"][k].shape != a["class_chi2"][k].shape:
                return math.inf, 0.0
            if a["class_chi2"][k].size:
                spread = max(spread, float(np.abs(r["class_chi2"][k] - a["class_chi2"][k]).max()))
                margin = min(margin, float(np.abs(r["class_chi2"][k] - float(f32(TH2))).min()))
    return spread, margin


def admissible(n_corr, kind, sc, results):
    """The condition on a test scene, on the model alone (results: variants(sc)).  The variants agree on every discrete result and took
    the same accept / reject path through the Levenberg loops, trial by trial, as far as a trial moves the estimate by NOISE_STEP or
    more (max |x_j|; below that it does not matter which way a decision falls, and it does fall both ways: at convergence the sign of
    rho is rounding noise, and the noise of a central difference with a step of 1e-9 turns it).  No edge chi2 of either classification lies
    closer to th2 than 100 x the largest disagreement of the variants on such a chi2.  And the scene reaches the exit it was built for."""
    a = results[0]
    for r in results[1:]:
        if (r["rounds"], r["n_bad"], r["more_iterations"], r["ret"]) != (a["rounds"], a["n_bad"], a["more_iterations"], a["ret"]) or \
                (r["inlier"] != a["inlier"]).any():
            return False
    if any(firm_decisions(r) != firm_decisions(a) for r in results[1:]):
        return False
    spread, margin = class_spread(results)
    if not margin >= 100 * spread:
        return False
    rounds, more, counted = expected_exit(n_corr, kind)
    if a["rounds"] != rounds or (more is not None and a["more_iterations"] != more) or (a["ret"] > 0) != counted:
        return False
    if rounds == 2 and a["inlier"][sc["gross"]].any():
        return False
    if kind == "starved" and n_corr >= 10 and not (0 < a["inlier"].sum() < 10):
        return False
    return True


def seed_of(n_corr, kind):
    """the seeds of the tests: the first of base, base + 5000, ... whose scene is admissible (tools/sim3opt_spread.py --select finds the
    shifts; tests/test_sim3opt_model.py checks every one of them)"""
    return 1000 * KINDS.index(kind) + n_corr + 5000 * SEED_SHIFT.get((n_corr, kind), 0)


SEED_SHIFT = {(1, 'outliers'): 9, (9, 'outliers'): 1, (10, 'clean'): 5, (11, 'outliers'): 7, (63, 'outliers'): 1, (64, 'clean'): 1, (64, 'starved'): 1,
              (257, 'outliers'): 1}
# a scene whose second round ends on a REJECTED trial: the classification then runs on the rejected estimate (tools/sim3opt_spread.py --select)
STALE_CASE = (65, "outliers", 90128)


# a start whose quaternion is NOT a unit one (norm 1.01): g2o::Sim3 never normalises, so the estimate keeps the norm it was handed, and an
# implementation that normalises after operator* shows.  The closed-form variant is left out of this one scene: it takes the derivative
# of rotating by exp(u).r * S.r as that of rotating twice, which Eigen's q * v formula does only for a unit quaternion.
NONUNIT_CASE = (65, "outliers")
NONUNIT_NORM = 1.01
EXTRA = ("stale", "nonunit")


def make_extra(name):
    if name == "stale":
        return make(*STALE_CASE)
    sc = make(*NONUNIT_CASE)
    sc["S12"] = sc["S12"].copy()
    sc["S12"][:4] *= NONUNIT_NORM
    sc["variants"] = tuple(v for v in VARIANTS if "jacobian" not in v)
    return sc


def extra_kind(name):
    return STALE_CASE[1] if name == "stale" else NONUNIT_CASE[1]


def make(n_corr, kind, seed=None):
    fix, unit = case_flags(n_corr, kind)
    return scene(seed_of(n_corr, kind) if seed is None else seed, n_corr, kind, fix_scale=fix, unit_start=unit)


CASES = [(n, kind) for n in N_CORR for kind in KINDS]


def all_scenes():
    return [(n, kind, make(n, kind)) for n, kind in CASES] + [(65, name, make_extra(name)) for name in EXTRA]
