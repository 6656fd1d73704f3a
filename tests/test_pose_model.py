"""tests/pose_model.py, the numpy restatement of Optimizer::PoseOptimization that the GPU tests compare with: its Jacobians against central
differences of its own error through its own exp / compose, convergence on noise-free scenes, known answers, the stale-error quirk of
g2o's pop(), and the condition on the GPU tests' scenes (checked here, on the CPU, so that tests/test_pose_opt.py never meets a scene
that hides a mismatch)."""
import math

import numpy as np
import pytest

import pose_model as pm
import pose_scene as ps
from tools.pose_spread import ORDERS, chi2_diff, pose_diff

f32 = np.float32


def _fd_error(mix, h):
    sc = ps.scene(7, 40, mix, outlier_frac=0.0, behind=False)
    E = pm.Edges(sc["obs"], sc["cam"])
    pose = pm.pose_from_Tcw(sc["Tcw"])
    A = E.jacobians(E.errors(pose)[0])
    worst = 0.0
    for j in range(6):
        d = np.zeros(6); d[j] = h
        fd = (E.errors(pm.oplus(pose, d))[1] - E.errors(pm.oplus(pose, -d))[1]) / (2 * h)
        worst = max(worst, float(np.abs(fd - A[:, :, j]).max()))
    return worst / float(np.abs(A).max()), float(np.abs(A).max())


def test_monocular_jacobian_against_central_differences():
    """g2o's analytic Jacobian is d(error)/d(x) with the update exp(x) * pose.  h = 1e-5: the measured disagreement is 1.07e-10 of the
    largest entry (1284), the truncation term ~ h^2 = 1e-10 (it falls as h^2 down to this h: 1.03e-4, 1.03e-6, 1.03e-8 at h = 1e-2 ..
    1e-4) plus rounding 2^-52 * 1241 px / h / 1284 = 2e-11; the tolerance is their sum 1.2e-10 doubled"""
    err, amax = _fd_error("mono", 1e-5)
    print(f"monocular Jacobian: central differences differ by {err:.3e} of the largest entry {amax:.1f}")
    assert err <= 2.4e-10
    assert _fd_error("mono", 1e-3)[0] > 1e-7                                   # and the test can see an error of 1e-6 of the largest entry


def test_stereo_jacobian_against_central_differences():
    """the stereo projection keeps invz in a float (types_six_dof_expmap.cpp:300), so its error is a staircase of relative height 2^-24:
    central differences see 2^-24 * 1241 px / (2 h) of noise on top of the truncation term.  h = 1e-3 balances them: measured 1.53e-5 of
    the largest entry; the tolerance is the staircase bound 2^-24 * 1241 / 1e-3 / 1284 = 5.8e-5 plus the truncation 1.0e-6"""
    err, amax = _fd_error("stereo", 1e-3)
    print(f"stereo Jacobian: central differences differ by {err:.3e} of the largest entry {amax:.1f}")
    assert err <= 2.0 ** -24 * 1241 / 1e-3 / amax + 1.1e-6
    # the Jacobian itself uses the double 1 / z: rows 0 and 1 of a stereo edge equal the monocular edge's
    sc = ps.scene(7, 40, "stereo", outlier_frac=0.0, behind=False)
    mono = dict(sc["obs"], u_right=np.full(len(sc["octave"]), -1, f32))
    Es, Em = pm.Edges(sc["obs"], sc["cam"]), pm.Edges(mono, sc["cam"])
    pose = pm.pose_from_Tcw(sc["Tcw"])
    assert (Es.jacobians(Es.errors(pose)[0])[:, :2] == Em.jacobians(Em.errors(pose)[0])[:, :2]).all()
    assert (Es.errors(pose)[1][:, :2] != Em.errors(pose)[1][:, :2]).any()     # while the errors differ: float invz against x / z


@pytest.mark.parametrize("mix", ps.MIXES)
def test_noise_free_scene_converges_back(mix):
    """exact measurements of float32 points, start 1.5 degrees / 0.15 units off: the pose comes back to the truth up to the float32 rounding
    of the inputs (points 2^-24 * 30 units, pixels 2^-24 * 1241 px = 7e-5 px over f / z >= 24 px per unit).  Measured: rotation 1.5e-9 ..
    4.3e-9, translation 2.9e-8 .. 5.6e-8; the tolerances are 2^-24 (rotation) and 2^-24 * 30 (translation, the depth range)"""
    sc = ps.scene(11, 80, mix, outlier_frac=0.0, behind=False, noise=False)
    r = pm.optimize(sc["obs"], sc["cam"], sc["Tcw"])
    T = sc["Tcw_true"]
    dR, dt = float(np.abs(r["pose"][:, :3] - T[:3, :3]).max()), float(np.abs(r["pose"][:, 3] - T[:3, 3]).max())
    d0 = float(np.abs(sc["Tcw"][:3].astype(np.float64) - T[:3]).max())
    print(f"{mix}: start off by {d0:.2e}, end rotation {dR:.2e} translation {dt:.2e}")
    assert d0 > 1e-2 and dR <= 2.0 ** -24 and dt <= 2.0 ** -24 * 30
    assert r["rounds"] == 4 and r["ret"] >= 79                                 # (a stereo feature clamped at u_right = 0 may go)


def test_huber_known_answers():
    d = pm.DELTA_MONO
    assert d == float(f32(math.sqrt(5.991))) and pm.DELTA_STEREO == float(f32(math.sqrt(7.815)))
    rho0, rho1 = pm.huber(np.array([0.0, 1.0, d * d, 4.0 * d * d]), d)
    assert rho0[0] == 0.0 and rho0[1] == 1.0 and rho0[2] == d * d and (rho1[:3] == 1.0).all()
    assert rho0[3] == 2.0 * (2.0 * d) * d - d * d == 3.0 * d * d and rho1[3] == d / (2.0 * d) == 0.5
    assert d * d != 5.991                                                      # the float delta squared in double is not the threshold


def test_fewer_than_three_correspondences():
    sc = ps.scene(3, 2, "mixed")
    r = pm.optimize(sc["obs"], sc["cam"], sc["Tcw"])
    assert r["ret"] == 0 and r["rounds"] == 0 and r["n_corr"] == 2 and not r["outlier"].any()
    assert r["Tcw"].tobytes() == sc["Tcw"].tobytes() and r["pose"].astype(f32).tobytes() == sc["Tcw"][:3].tobytes()
    r = pm.optimize(ps.scene(3, 0, "mixed")["obs"], sc["cam"], sc["Tcw"])
    assert r["ret"] == 0 and r["n_corr"] == 0


def test_fewer_than_ten_edges_stop_after_one_round():
    for n, rounds in ((3, 1), (9, 1), (10, 4)):
        sc = ps.scene(ps.seed_of(n, "mixed"), n, "mixed")
        r = pm.optimize(sc["obs"], sc["cam"], sc["Tcw"])
        assert r["rounds"] == rounds and len(r["flags"]) == rounds and r["ret"] == n - r["n_bad"][rounds - 1]
        assert r["n_bad"][rounds:] == [0] * (4 - rounds) and r["iterations"][rounds:] == [0] * (4 - rounds)


def test_every_round_restarts_from_the_input_pose():
    sc = ps.scene(ps.seed_of(64, "mixed"), 64, "mixed")
    first = []
    pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], hook=lambda it, i, q, acc, pose: first.append((it, pose)) if i == 0 and q == 0 else None)
    assert [f[0] for f in first] == [0, 1, 2, 3]
    # the first trial of rounds 1 and 2 starts from the same pose with the same robust kernels but fewer edges: a different step; had the
    # round started from the previous round's (converged) pose, its first step would be tiny
    start = pm.pose_from_Tcw(sc["Tcw"])
    for _, pose in first:
        assert np.abs(pose[1] - start[1]).max() > 1e-2


def test_stale_error_of_a_rejected_last_trial():
    """g2o's pop() restores the vertex, not the edge errors: when the last trial of a round is rejected, the active edges are classified by
    their errors at the REJECTED pose.  Constructed: 9 points, half of them stereo (one round; the float invz of the stereo projection makes chi2 a staircase
    on which the last iteration's ten trials are all rejected), so the loop ends on a rejected trial; the chi2 the
    classification used is, bit for bit, the one at the rejected trial's pose and not the one at the pose the round returns"""
    sc = ps.scene(50, 9, "mixed")
    trials = []
    r = pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], hook=lambda it, i, q, acc, pose: trials.append((acc, pose)))
    assert r["stale_used"] and r["rounds"] == 1 and trials[-1][0] is False
    E = pm.Edges(sc["obs"], sc["cam"])
    rejected = E.errors(trials[-1][1])[2]
    last_accepted = [p for a, p in trials if a][-1]
    kept = E.errors(last_accepted)[2]
    used = r["class_chi2"][0]
    print("chi2 used", used, "at the rejected pose", rejected, "at the restored pose", kept)
    assert used.tobytes() == rejected.tobytes() and np.abs(used - kept).max() > 1e-8      # measured 7.3e-08
    assert np.abs(pm.quat_to_matrix(last_accepted[0]) - r["pose"][:, :3]).max() == 0.0   # while the pose returned is the restored one


def test_scenes_of_the_gpu_tests_satisfy_their_condition():
    """every (size, mix) scene: admissible on the model, and the model's three orders within the spread that tests/test_pose_opt.py and
    DESIGN.md state (python tools/pose_spread.py prints the same figures)"""
    import test_pose_opt as tp
    worst_p = worst_c = 0.0
    for n, mix, sc in ps.all_scenes():
        rs = [pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], o) for o in ORDERS]
        assert ps.admissible(n, sc, rs), (n, mix)
        worst_p = max(worst_p, max(pose_diff(rs[0]["pose"], r["pose"]) for r in rs[1:]))
        worst_c = max(worst_c, max(chi2_diff(rs[0]["chi2"], r["chi2"]) for r in rs[1:]))
    print(f"spread over the scenes: pose {worst_p:.3e} chi2 {worst_c:.3e}")
    assert worst_p <= tp.SPREAD_POSE and worst_c <= tp.SPREAD_CHI2
    assert 64 * max(tp.SPREAD_POSE, tp.SPREAD_CHI2) < 1e-9
    assert worst_p >= 0.99 * tp.SPREAD_POSE and worst_c >= 0.99 * tp.SPREAD_CHI2   # the constants are the measurement, not a looser figure


def test_chain_scene_satisfies_its_condition(oracle):
    """the scene of test_pose_opt.test_chain_search_then_optimise, with the matches the CPU oracle's search finds (tests/test_local_points.py
    pins the device search to them)"""
    import frustum_model as fm
    import localmap_scene as ls
    import test_pose_opt as tp
    frame, geom, desc, slots, flags, po, Tcw, isig = tp.chain_world(ls)
    exp = fm.frustum(geom, flags & 1, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    pts = dict(u=exp["u"], v=exp["v"], aux=exp["xr"], level=exp["level"], angle=np.zeros(len(geom), f32), view_cos=exp["view_cos"], desc=desc,
               valid=exp["in_view"], has_obs=(flags >> 1) & 1)
    match, _ = oracle.search_by_projection_points(dict(frame, occupied=np.zeros(len(frame["x"]), np.uint8)), pts, ls.SF, 3.0, 0.8)
    slot = tp.chain_inputs(match, ls, frame, slots)
    by_slot = np.zeros((512, 8), f32); by_slot[slots] = geom
    obs = tp.chain_obs(frame, by_slot[slot[slot >= 0]], slot, isig)
    rs = [pm.optimize(obs, ls.CAM[:5], Tcw, o) for o in ORDERS]
    assert rs[0]["n_corr"] > 40 and rs[0]["rounds"] == 4
    assert ps.admissible(0, dict(gross=np.zeros(len(slot), bool)), rs)
    assert max(pose_diff(rs[0]["pose"], r["pose"]) for r in rs[1:]) <= tp.SPREAD_POSE
