"""orbx_pose_optimize, orbx_local_bundle_adjustment and orbx_bundle_adjustment in TURNED world frames (tests/turned_frames.py): the three
solvers that take a float Tcw and convert it on the device (quat_from_matrix and quat_normalize of orbx_lm.h, called by k_pose_opt and
k_lba_init).  The scenes of test_pose_opt.py, test_lba.py and test_gba.py reach only the trace > 0 branch of that conversion; these reach
the other three, the tie rule and the sign flip.

Exact layer (no Levenberg step): keyframes without edges come back as the quaternion round trip of their float matrix, byte for byte
against the model; the device code is built with -ffp-contract=off, and double sqrt and division are correctly rounded.
Against the model: the checks of the three solver tests, every exact field exact, under bounds MEASURED on the turned scenes:

    python tools/turned_spread.py
    POSE_SPREAD_POSE = 3.894e-15  POSE_SPREAD_CHI2 = 1.436e-13  (x 64: 2.492e-13, 9.190e-12)
    LBA_SPREAD_POSE = 3.701e-13  LBA_SPREAD_POINT = 9.105e-14  LBA_SPREAD_CHI2 = 4.287e-13  (x 64: 2.369e-11, 5.827e-12, 2.744e-11)
    GBA_SPREAD_POSE = 7.984e-14  GBA_SPREAD_POINT = 1.395e-12  GBA_SPREAD_CHI2 = 3.265e-14  (x 64: 5.110e-12, 8.928e-11, 2.090e-12)

the largest disagreement of each model with itself across its three summation orders over the turned scenes, in the metrics of
tools/pose_spread.py and tools/lba_spread.py.  The GPU gets 64 x that spread, the project's standing margin for a fourth reduction tree
and the device's sin and cos.  What the bounds must not hide is a wrong branch:

    python tools/turned_spread.py --mutations
    MUTATION quat_branch1 pose smallest change 1.704e-07 over 12 scenes
    MUTATION quat_branch2 pose smallest change 7.382e-07 over 13 scenes
    MUTATION quat_branch3 pose smallest change 3.103e-07 over 14 scenes
    MUTATION quat_branch1 lba smallest change 2.461e-03 over 14 scenes
    MUTATION quat_branch2 lba smallest change 1.553e-02 over 14 scenes
    MUTATION quat_branch3 lba smallest change 6.795e-01 over 17 scenes
    MUTATION quat_branch1 gba smallest change 1.471e-02 over 7 scenes
    MUTATION quat_branch2 gba smallest change 2.004e-02 over 8 scenes
    MUTATION quat_branch3 gba smallest change 3.574e-03 over 9 scenes
    MUTATION quat_tie_ge changes the round trip of 3 of 3 tie matrices
    MUTATION quat_no_flip largest change pose 0.000e+00 lba 0.000e+00 gba 0.000e+00   (q and -q are one rotation: the flip is exercised,
                                                                                        and not observable through these entry points)

and BOUND <= SMALLEST_MUTATION / 16 is asserted below.  tests/test_turned_frames_model.py holds the scenes' conditions and both halves of
the mutation argument on the model alone.
Metamorphic (half turns, exact in float): the device's result on the turned scene, turned back, is its result on the un-turned scene of
the same seed: every discrete field identical, the estimates within 2 x the bound; each side is also held to one bound of its own model
run.  On the MI355X the largest differences from the model were 4.8e-15 (pose) and 8.4e-14 (chi2) for pose optimisation, 2.4e-13 /
7.3e-14 / 3.2e-13 (pose / point / chi2) for LBA and 3.4e-14 / 5.6e-13 / 1.8e-14 for GBA.  The two problems differ in the rounding of their first quaternion, and a few Levenberg iterations do not forget a start entirely:
the model's own two runs are up to 4.2e-13 (pose, 65-mono-piz), 2.5e-13 (LBA pose) and 1.1e-12 (GBA point) apart, printed per case."""
import numpy as np
import pytest

import gba_model as gm
import gba_scene as gs
import lba_model as lm
import lba_scene as ls
import pose_model as pm
import pose_scene as ps
import turned_frames as tf
from test_pose_opt import _frame_dict, _table
from tools.lba_spread import points_diff, poses_diff
from tools.pose_spread import ORDERS, chi2_diff, pose_diff

f32 = np.float32
POSE_SPREAD_POSE, POSE_SPREAD_CHI2 = 3.894e-15, 1.436e-13                                  # python tools/turned_spread.py
LBA_SPREAD_POSE, LBA_SPREAD_POINT, LBA_SPREAD_CHI2 = 3.701e-13, 9.105e-14, 4.287e-13
GBA_SPREAD_POSE, GBA_SPREAD_POINT, GBA_SPREAD_CHI2 = 7.984e-14, 1.395e-12, 3.265e-14
POSE_BOUND = dict(pose=64 * POSE_SPREAD_POSE, chi2=64 * POSE_SPREAD_CHI2)
LBA_BOUND = dict(pose=64 * LBA_SPREAD_POSE, point=64 * LBA_SPREAD_POINT, chi2=64 * LBA_SPREAD_CHI2)
GBA_BOUND = dict(pose=64 * GBA_SPREAD_POSE, point=64 * GBA_SPREAD_POINT, chi2=64 * GBA_SPREAD_CHI2)
POSE_SMALLEST_MUTATION = 1.704e-07                                                         # python tools/turned_spread.py --mutations
LBA_SMALLEST_MUTATION = 2.461e-03
GBA_SMALLEST_MUTATION = 3.574e-03
assert max(POSE_BOUND.values()) <= POSE_SMALLEST_MUTATION / 16, "the bound could hide a wrong branch"
assert max(LBA_BOUND.values()) <= LBA_SMALLEST_MUTATION / 16, "the bound could hide a wrong branch"
assert max(GBA_BOUND.values()) <= GBA_SMALLEST_MUTATION / 16, "the bound could hide a wrong branch"

_cache = {}


def memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def pose_runs(sc):
    return memo(("pose", id(sc)), lambda: (sc, [pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], o) for o in ORDERS]))[1]


def lba_runs(sc):
    return memo(("lba", id(sc)), lambda: (sc, [lm.optimize(sc["problem"], o) for o in lm.ORDERS]))[1]


def gba_runs(sc, opts):
    return memo(("gba", id(sc)), lambda: (sc, [gm.optimize(sc["problem"], order=o, **opts) for o in gm.ORDERS]))[1]


def same_bytes(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def round_trip(M):
    """the model's conversion of a float rotation block to a quaternion and back, in double"""
    return pm.quat_to_matrix(pm.quat_normalize(pm.quat_from_matrix(np.asarray(M, f32).astype(np.float64))))


# ---------------------------------------------------------------- the exact layer

def check_exact(got, pr):
    Tin = np.asarray(pr["Tcw"], f32)
    for k, (name, M, _, _) in enumerate(tf.EXACT_ROTATIONS):
        exp = np.concatenate([round_trip(M), Tin[k, :3, 3:].astype(np.float64)], axis=1)
        assert np.isfinite(exp).all()
        assert got["pose"][k].tobytes() == exp.tobytes(), (name, got["pose"][k], exp)
    assert got["Tcw"][:, :3].tobytes() == got["pose"].astype(f32).tobytes()
    assert (got["Tcw"][:, 3] == np.array([0, 0, 0, 1], f32)).all()
    assert got["Xw"].tobytes() == np.asarray(pr["Xw"], f32).tobytes()


@pytest.mark.gpu
def test_exact_rotations_through_bundle_adjustment(pkg):
    pr = tf.exact_problem()
    got = pkg.bundle_adjustment(pr, iterations=0)
    assert (got["iterations"], got["trials"], got["stopped"], got["n_active_kf"]) == (0, 0, 0, 0)
    check_exact(got, pr)
    assert same_bytes(got, pkg.bundle_adjustment(pr, iterations=0))
    check_exact(pkg.bundle_adjustment(pr, iterations=10), pr)              # no edge: ten iterations move nothing either


@pytest.mark.gpu
def test_exact_rotations_through_local_bundle_adjustment(pkg):
    pr = tf.exact_problem(fixed_half=True)
    assert 0 < int(pr["fixed"].sum()) < len(pr["fixed"])
    got = pkg.local_bundle_adjustment(pr)
    assert got["n_active_kf"] == [0, 0] and got["trials"] == [0, 0] and got["stopped"] == 0
    check_exact(got, pr)
    assert same_bytes(got, pkg.local_bundle_adjustment(pr))


# ---------------------------------------------------------------- against the model

def check_pose(got, exp, Tcw_in, tag, bound=POSE_BOUND):
    """test_pose_opt.check_against_model under the turned bounds"""
    margin = min([float(m.min()) for m in exp["margin"] if len(m)] or [1.0])
    dp, dc = pose_diff(exp["pose"], got["pose"]), chi2_diff(exp["chi2"], got["chi2"])
    print(f"pose {tag}: branch {tf.branch_of(np.asarray(Tcw_in)[:3, :3])} n_corr {got['n_corr']} rounds {got['rounds']} n_bad {list(got['n_bad'])} iterations "
          f"{list(got['iterations'])} model {exp['iterations']} flips {exp['quat_flips']} margin {margin:.2e} pose {dp:.3e} (bound {bound['pose']:.3e}) "
          f"chi2 {dc:.3e} (bound {bound['chi2']:.3e})")
    assert margin >= 1e-6, "the scene has an edge within 1e-6 of its threshold: replace it"
    assert got["n_corr"] == exp["n_corr"] and got["rounds"] == exp["rounds"] and list(got["n_bad"]) == exp["n_bad"]
    assert got["n_inliers"] == exp["ret"]
    assert got["outlier"].tobytes() == exp["outlier"].tobytes(), np.nonzero(got["outlier"] != exp["outlier"])[0][:8]
    assert got["Tcw"].tobytes() == np.concatenate([got["pose"].astype(f32), [[0, 0, 0, 1]]]).astype(f32).tobytes()
    assert dp <= bound["pose"] and dc <= bound["chi2"]


def check_lba(got, exp, pr, tag, bound=LBA_BOUND):
    """test_lba.check_against_model under the turned bounds"""
    dp, dx, dc = poses_diff(exp["pose"], got["pose"]), points_diff(exp["point"], got["point"]), chi2_diff(exp["chi2"], got["chi2"])
    print(f"lba {tag}: branches {sorted(set(tf.branches_of_problem(pr)))} active kf {got['n_active_kf']} points {got['n_active_points']} iterations "
          f"{got['iterations']} model {exp['iterations']} trials {got['trials']} model {exp['trials']} level1 {got['n_level1']} erase {got['n_erase']} "
          f"flips {exp['quat_flips']} pose {dp:.3e} (bound {bound['pose']:.3e}) point {dx:.3e} (bound {bound['point']:.3e}) chi2 {dc:.3e} "
          f"(bound {bound['chi2']:.3e})")
    assert exp["margin_chi2"] >= ls.MARGIN and exp["margin_depth"] >= ls.MARGIN, "the scene has an edge within 1e-6 of a threshold: replace it"
    assert got["stopped"] == exp["stopped"]
    assert got["edge_flags"].tobytes() == exp["edge_flags"].tobytes(), np.nonzero(got["edge_flags"] != exp["edge_flags"])[0][:8]
    assert (got["n_level1"], got["n_erase"]) == (exp["n_level1"], exp["n_erase"])
    assert got["n_active_kf"] == exp["n_active_kf"] and got["n_active_points"] == exp["n_active_points"]
    assert got["Tcw"][:, :3].tobytes() == got["pose"].astype(f32).tobytes() and got["Xw"].tobytes() == got["point"].astype(f32).tobytes()
    assert (got["Tcw"][:, 3] == np.array([0, 0, 0, 1], f32)).all()
    for k in np.nonzero(pr["fixed"])[0]:                                   # the quaternion round trip of the input, exactly
        assert got["pose"][k].tobytes() == exp["pose"][k].tobytes(), k
        assert got["pose"][k, :, :3].tobytes() == round_trip(pr["Tcw"][k][:3, :3]).tobytes(), k
    deg = np.bincount(pr["edge_point"], minlength=len(pr["Xw"]))
    assert got["Xw"][deg == 0].tobytes() == np.asarray(pr["Xw"], f32)[deg == 0].tobytes()
    assert dp <= bound["pose"] and dx <= bound["point"] and dc <= bound["chi2"]


def check_gba(got, exp, pr, tag, bound=GBA_BOUND):
    """test_gba.check_against_model under the turned bounds"""
    dp, dx, dc = poses_diff(exp["pose"], got["pose"]), points_diff(exp["point"], got["point"]), chi2_diff(exp["chi2"], got["chi2"])
    print(f"gba {tag}: branches {sorted(set(tf.branches_of_problem(pr)))} active kf {got['n_active_kf']} points {got['n_active_points']} iterations "
          f"{got['iterations']} model {exp['iterations']} trials {got['trials']} model {exp['trials']} chi2 {got['chi2']:.6g} flips {exp['quat_flips']} "
          f"pose {dp:.3e} (bound {bound['pose']:.3e}) point {dx:.3e} (bound {bound['point']:.3e}) chi2 {dc:.3e} (bound {bound['chi2']:.3e})")
    assert got["stopped"] == exp["stopped"]
    assert got["n_active_kf"] == exp["n_active_kf"] and got["n_active_points"] == exp["n_active_points"]
    assert got["point_included"].tobytes() == exp["point_included"].tobytes()
    assert got["Tcw"][:, :3].tobytes() == got["pose"].astype(f32).tobytes() and got["Xw"].tobytes() == got["point"].astype(f32).tobytes()
    assert (got["Tcw"][:, 3] == np.array([0, 0, 0, 1], f32)).all()
    has_edge = np.zeros(len(pr["fixed"]), bool)
    has_edge[pr["edge_kf"]] = True
    for k in np.nonzero((np.asarray(pr["fixed"]) != 0) | ~has_edge)[0]:    # no row: the quaternion round trip of the input, exactly
        assert got["pose"][k].tobytes() == exp["pose"][k].tobytes(), k
        assert got["pose"][k, :, :3].tobytes() == round_trip(pr["Tcw"][k][:3, :3]).tobytes(), k
    out = got["point_included"] == 0
    assert got["Xw"][out].tobytes() == np.asarray(pr["Xw"], f32).reshape(-1, 3)[out].tobytes()
    assert dp <= bound["pose"] and dx <= bound["point"] and dc <= bound["chi2"]


def pose_world(n, mix, turn):
    return memo(("pose case", n, mix, turn), lambda: tf.pose_case(n, mix, turn))


def lba_world(shape, mix, turn):
    return memo(("lba case", shape, mix, turn), lambda: tf.lba_case(shape, mix, turn))


def gba_world(shape, turn):
    return memo(("gba case", shape, turn), lambda: tf.gba_case(shape, turn))


@pytest.mark.gpu
@pytest.mark.parametrize("n,mix,turn", tf.POSE_CASES, ids=[tf.pose_tag(*c) for c in tf.POSE_CASES])
def test_pose_matches_the_model(pkg, n, mix, turn):
    sc = pose_world(n, mix, turn)
    rs = pose_runs(sc)
    assert ps.admissible(n, sc, rs), "the scene does not satisfy its condition on the model: replace it (tools/turned_spread.py --select)"
    if turn != "d22":
        assert tf.branch_of(sc["Tcw"][:3, :3]) == tf.TURN_BRANCH[turn]
    got = pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])
    check_pose(got, rs[0], sc["Tcw"], tf.pose_tag(n, mix, turn))
    assert got["rounds"] == 4 and got["outlier"][sc["gross"]].all()        # the point behind the camera among them
    assert same_bytes(got, pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mix,turn", tf.LBA_CASES, ids=[tf.lba_tag(*c) for c in tf.LBA_CASES])
def test_lba_matches_the_model(pkg, shape, mix, turn):
    sc = lba_world(shape, mix, turn)
    rs = lba_runs(sc)
    assert ls.admissible(sc, rs), "the scene does not satisfy its condition on the model: replace it (tools/turned_spread.py --select)"
    if turn != "d22":
        assert set(tf.branches_of_problem(sc["problem"])) == {tf.TURN_BRANCH[turn]}
    got = pkg.local_bundle_adjustment(sc["problem"])
    check_lba(got, rs[0], sc["problem"], tf.lba_tag(shape, mix, turn))
    assert same_bytes(got, pkg.local_bundle_adjustment(sc["problem"]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,turn", tf.GBA_CASES, ids=[tf.gba_tag(*c) for c in tf.GBA_CASES])
def test_gba_matches_the_model(pkg, shape, turn):
    sc, opts = gba_world(shape, turn)
    rs = gba_runs(sc, opts)
    assert gs.admissible(rs), "the scene does not satisfy its condition on the model: replace it (tools/turned_spread.py --select)"
    if turn != "d22":
        assert set(tf.branches_of_problem(sc["problem"])) == {tf.TURN_BRANCH[turn]}
    got = pkg.bundle_adjustment(sc["problem"], **opts)
    check_gba(got, rs[0], sc["problem"], tf.gba_tag(shape, turn))
    assert same_bytes(got, pkg.bundle_adjustment(sc["problem"], **opts))


# ---------------------------------------------------------------- metamorphic: the exact half turns

HALF_POSE = [c for c in tf.POSE_CASES if c[2] in tf.HALF_TURNS]
HALF_LBA = [c for c in tf.LBA_CASES if c[2] in tf.HALF_TURNS]
HALF_GBA = [c for c in tf.GBA_CASES if c[1] in tf.HALF_TURNS]


def test_a_half_turn_flips_signs_and_nothing_else():
    """what makes the metamorphic comparison exact on the input side: the turned floats are the un-turned ones up to their sign"""
    t, u = tf.pose_pair(65, "stereo", "piy")
    assert np.abs(t["Tcw"]).tobytes() == np.abs(u["Tcw"]).tobytes() and np.abs(t["obs"]["Xw"]).tobytes() == np.abs(u["obs"]["Xw"]).tobytes()
    assert (t["Tcw"][:3, :3] == u["Tcw"][:3, :3] @ tf.TURNS["piy"].astype(f32)).all() and (t["Tcw"][:, 3] == u["Tcw"][:, 3]).all()
    t, u = tf.lba_pair((3, 2, 64), "mixed", "piz")
    assert np.abs(t["problem"]["Tcw"]).tobytes() == np.abs(u["problem"]["Tcw"]).tobytes()
    assert np.abs(t["problem"]["Xw"]).tobytes() == np.abs(u["problem"]["Xw"]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n,mix,turn", HALF_POSE, ids=[tf.pose_tag(*c) for c in HALF_POSE])
def test_pose_half_turn_is_the_same_problem(pkg, n, mix, turn):
    t, u = memo(("pose pair", n, mix, turn), lambda: tf.pose_pair(n, mix, turn))
    assert ps.admissible(n, t, pose_runs(t)) and ps.admissible(n, u, pose_runs(u)), "replace the pair (tools/turned_spread.py --select)"
    gt, gu = pkg.pose_optimize(t["obs"], t["cam"], t["Tcw"]), pkg.pose_optimize(u["obs"], u["cam"], u["Tcw"])
    check_pose(gt, pose_runs(t)[0], t["Tcw"], tf.pose_tag(n, mix, turn) + " pair, turned")
    check_pose(gu, pose_runs(u)[0], u["Tcw"], tf.pose_tag(n, mix, turn) + " pair, un-turned")
    G = tf.TURNS[turn]
    dp, dc = pose_diff(gu["pose"], tf.turn_back_pose(gt["pose"], G)), chi2_diff(gu["chi2"], gt["chi2"])
    mp = pose_diff(pose_runs(u)[0]["pose"], tf.turn_back_pose(pose_runs(t)[0]["pose"], G))
    print(f"pose pair {tf.pose_tag(n, mix, turn)}: iterations {list(gt['iterations'])} un-turned {list(gu['iterations'])} pose {dp:.3e} "
          f"(2 x bound {2 * POSE_BOUND['pose']:.3e}; the model's two runs {mp:.3e}) chi2 {dc:.3e} (2 x bound {2 * POSE_BOUND['chi2']:.3e})")
    assert gt["outlier"].tobytes() == gu["outlier"].tobytes() and list(gt["n_bad"]) == list(gu["n_bad"])
    assert (gt["rounds"], gt["n_corr"], gt["n_inliers"]) == (gu["rounds"], gu["n_corr"], gu["n_inliers"])
    assert dp <= 2 * POSE_BOUND["pose"] and dc <= 2 * POSE_BOUND["chi2"]


def _ba_pair_check(tag, gt, gu, mt, mu, G, bound, exact):
    dp = poses_diff(gu["pose"], tf.turn_back_pose(gt["pose"], G))
    dx = points_diff(gu["point"], tf.turn_back_points(gt["point"], G))
    dc = chi2_diff(gu["chi2"], gt["chi2"])
    mp, mx = poses_diff(mu["pose"], tf.turn_back_pose(mt["pose"], G)), points_diff(mu["point"], tf.turn_back_points(mt["point"], G))
    print(f"{tag}: trials {gt['trials']} un-turned {gu['trials']} pose {dp:.3e} (2 x bound {2 * bound['pose']:.3e}; the model's two runs {mp:.3e}) "
          f"point {dx:.3e} (2 x bound {2 * bound['point']:.3e}; the model's {mx:.3e}) chi2 {dc:.3e} (2 x bound {2 * bound['chi2']:.3e})")
    for k in exact:
        assert np.asarray(gt[k]).tobytes() == np.asarray(gu[k]).tobytes(), k
    assert dp <= 2 * bound["pose"] and dx <= 2 * bound["point"] and dc <= 2 * bound["chi2"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mix,turn", HALF_LBA, ids=[tf.lba_tag(*c) for c in HALF_LBA])
def test_lba_half_turn_is_the_same_problem(pkg, shape, mix, turn):
    t, u = memo(("lba pair", shape, mix, turn), lambda: tf.lba_pair(shape, mix, turn))
    assert ls.admissible(t, lba_runs(t)) and ls.admissible(u, lba_runs(u)), "replace the pair (tools/turned_spread.py --select)"
    gt, gu = pkg.local_bundle_adjustment(t["problem"]), pkg.local_bundle_adjustment(u["problem"])
    check_lba(gt, lba_runs(t)[0], t["problem"], tf.lba_tag(shape, mix, turn) + " pair, turned")
    check_lba(gu, lba_runs(u)[0], u["problem"], tf.lba_tag(shape, mix, turn) + " pair, un-turned")
    _ba_pair_check("lba pair " + tf.lba_tag(shape, mix, turn), gt, gu, lba_runs(t)[0], lba_runs(u)[0], tf.TURNS[turn], LBA_BOUND,
                   ("edge_flags", "n_level1", "n_erase", "n_active_kf", "n_active_points", "stopped"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,turn", HALF_GBA, ids=[tf.gba_tag(*c) for c in HALF_GBA])
def test_gba_half_turn_is_the_same_problem(pkg, shape, turn):
    t, u = memo(("gba pair", shape, turn), lambda: tf.gba_pair(shape, turn))
    opts = tf.gba_options(shape)
    assert gs.admissible(gba_runs(t, opts)) and gs.admissible(gba_runs(u, opts)), "replace the pair (tools/turned_spread.py --select)"
    gt, gu = pkg.bundle_adjustment(t["problem"], **opts), pkg.bundle_adjustment(u["problem"], **opts)
    check_gba(gt, gba_runs(t, opts)[0], t["problem"], tf.gba_tag(shape, turn) + " pair, turned")
    check_gba(gu, gba_runs(u, opts)[0], u["problem"], tf.gba_tag(shape, turn) + " pair, un-turned")
    _ba_pair_check("gba pair " + tf.gba_tag(shape, turn), gt, gu, gba_runs(t, opts)[0], gba_runs(u, opts)[0], tf.TURNS[turn], GBA_BOUND,
                   ("point_included", "n_active_kf", "n_active_points", "stopped"))


# ---------------------------------------------------------------- launch forms

def _batch_jobs():
    """seven jobs of sizes 65, 0, 2, 10, 64, 10, 63 whose start poses lie in all four branches"""
    plan = [(65, "mixed", "x3"), (0, "mono", "y3"), (2, "stereo", "z3"), (10, "stereo", "y3"), (64, "mono", "z3"), (10, "mixed", "piy"), (63, "stereo", None)]
    return [tf.pose_case(n, mix, turn) for n, mix, turn in plan]                   # a case of the table, or the first seed of its family


def test_batch_jobs_cover_the_branches():
    scs = _batch_jobs()
    assert [int(sc["obs"]["has_point"].sum()) for sc in scs] == [65, 0, 2, 10, 64, 10, 63]
    assert {tf.branch_of(sc["Tcw"][:3, :3]) for sc in scs} == {0, 1, 2, 3}


@pytest.mark.gpu
def test_batch_equals_the_single_calls(pkg):
    from test_pose_opt import same_bytes as same_pose
    scs = _batch_jobs()
    got = pkg.pose_optimize_batch([(sc["obs"], sc["cam"], sc["Tcw"]) for sc in scs])
    assert len(got) == 7
    for j, sc in enumerate(scs):
        assert same_pose(got[j], pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])), j
    assert got[1]["n_corr"] == 0 and got[2]["n_corr"] == 2 and got[0]["rounds"] == 4
    for j in (1, 2):                                                       # fewer than 3 correspondences: the float pose comes back as it went in
        assert got[j]["Tcw"].tobytes() == scs[j]["Tcw"].tobytes()


@pytest.mark.gpu
def test_resident_equals_host_pointers(pkg):
    from test_pose_opt import same_bytes as same_pose
    sc = pose_world(65, "mixed", "z3")
    assert tf.branch_of(sc["Tcw"][:3, :3]) == 3
    host = pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])
    df = pkg.DeviceFrame(_frame_dict(sc))
    mp, slot, _ = _table(pkg, sc)
    got = df.pose_optimize(mp, slot, ps.INV_SIGMA2, sc["cam"], sc["Tcw"])
    assert same_pose(got, host)
    assert same_pose(df.pose_optimize(mp, slot, ps.INV_SIGMA2, sc["cam"], sc["Tcw"]), host)
