"""tests/turned_frames.py on the models alone, without a GPU: every turned scene satisfies its solver's condition in the three summation
orders and stays within the spread tests/test_turned_frames.py builds its bounds on; the scenes reach what they are there for (each of
the branches 1, 2, 3 of Quaternion(Matrix3) per solver, three branches inside one d22 problem, a sign flip inside pose_mul); the exact
rotations take the branch they were built for and survive the conversion; and the two halves of the mutation argument: a wrong
trace <= 0 branch changes NO output of any scene of the existing solver tests, and changes every turned scene that uses the branch by
more than 16 x its bound."""
import math

import numpy as np
import pytest

import gba_model as gm
import gba_scene as gs
import lba_model as lm
import lba_scene as ls
import pose_model as pm
import pose_scene as ps
import turned_frames as tf
from test_turned_frames import (GBA_BOUND, GBA_SPREAD_CHI2, GBA_SPREAD_POINT, GBA_SPREAD_POSE, LBA_BOUND, LBA_SPREAD_CHI2, LBA_SPREAD_POINT,
                                LBA_SPREAD_POSE, POSE_BOUND, POSE_SPREAD_CHI2, POSE_SPREAD_POSE, gba_runs, lba_runs, memo, pose_runs, round_trip)
from tools.lba_spread import out_diff, points_diff, poses_diff
from tools.pose_spread import chi2_diff, pose_diff
from tools.turned_spread import finite, pose_out_diff

BRANCH_MUTATIONS = ("quat_branch1", "quat_branch2", "quat_branch3")
ULP_OF_ONE = 2.0 ** -52


def pose_world(n, mix, turn):
    sc = memo(("pose case", n, mix, turn), lambda: tf.pose_case(n, mix, turn))
    return sc, pose_runs(sc)


def lba_world(shape, mix, turn):
    sc = memo(("lba case", shape, mix, turn), lambda: tf.lba_case(shape, mix, turn))
    return sc, lba_runs(sc)


def gba_world(shape, turn):
    sc, opts = memo(("gba case", shape, turn), lambda: tf.gba_case(shape, turn))
    return sc, opts, gba_runs(sc, opts)


# ---------------------------------------------------------------- the scenes

@pytest.mark.parametrize("n,mix,turn", tf.POSE_CASES, ids=[tf.pose_tag(*c) for c in tf.POSE_CASES])
def test_pose_scene_is_admissible_and_orders_agree(n, mix, turn):
    sc, rs = pose_world(n, mix, turn)
    assert ps.admissible(n, sc, rs), "replace the scene (tools/turned_spread.py --select)"
    a = rs[0]
    dp = max(pose_diff(a["pose"], r["pose"]) for r in rs[1:])
    dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
    print(f"{tf.pose_tag(n, mix, turn)}: branch {tf.branch_of(sc['Tcw'][:3, :3])} flips {a['quat_flips']} self-disagreement pose {dp:.3e} chi2 {dc:.3e}")
    assert dp <= POSE_SPREAD_POSE and dc <= POSE_SPREAD_CHI2
    if turn != "d22":
        assert tf.branch_of(sc["Tcw"][:3, :3]) == tf.TURN_BRANCH[turn]
    if turn in tf.HALF_TURNS:
        t, u = tf.pose_pair(n, mix, turn)
        assert ps.admissible(n, t, pose_runs(t)) and ps.admissible(n, u, pose_runs(u)), "replace the pair (tools/turned_spread.py --select)"


@pytest.mark.parametrize("shape,mix,turn", tf.LBA_CASES, ids=[tf.lba_tag(*c) for c in tf.LBA_CASES])
def test_lba_scene_is_admissible_and_orders_agree(shape, mix, turn):
    sc, rs = lba_world(shape, mix, turn)
    assert ls.admissible(sc, rs), "replace the scene (tools/turned_spread.py --select)"
    a = rs[0]
    dp = max(poses_diff(a["pose"], r["pose"]) for r in rs[1:])
    dx = max(points_diff(a["point"], r["point"]) for r in rs[1:])
    dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
    print(f"{tf.lba_tag(shape, mix, turn)}: branches {tf.branches_of_problem(sc['problem'])} flips {a['quat_flips']} self-disagreement pose {dp:.3e} "
          f"point {dx:.3e} chi2 {dc:.3e}")
    assert dp <= LBA_SPREAD_POSE and dx <= LBA_SPREAD_POINT and dc <= LBA_SPREAD_CHI2
    if turn != "d22":
        assert set(tf.branches_of_problem(sc["problem"])) == {tf.TURN_BRANCH[turn]}
    if turn in tf.HALF_TURNS:
        t, u = tf.lba_pair(shape, mix, turn)
        assert ls.admissible(t, lba_runs(t)) and ls.admissible(u, lba_runs(u)), "replace the pair (tools/turned_spread.py --select)"


@pytest.mark.parametrize("shape,turn", tf.GBA_CASES, ids=[tf.gba_tag(*c) for c in tf.GBA_CASES])
def test_gba_scene_is_admissible_and_orders_agree(shape, turn):
    sc, opts, rs = gba_world(shape, turn)
    assert gs.admissible(rs), "replace the scene (tools/turned_spread.py --select)"
    a = rs[0]
    dp = max(poses_diff(a["pose"], r["pose"]) for r in rs[1:])
    dx = max(points_diff(a["point"], r["point"]) for r in rs[1:])
    dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
    print(f"{tf.gba_tag(shape, turn)}: branches {tf.branches_of_problem(sc['problem'])} flips {a['quat_flips']} self-disagreement pose {dp:.3e} "
          f"point {dx:.3e} chi2 {dc:.3e}")
    assert dp <= GBA_SPREAD_POSE and dx <= GBA_SPREAD_POINT and dc <= GBA_SPREAD_CHI2
    if turn != "d22":
        assert set(tf.branches_of_problem(sc["problem"])) == {tf.TURN_BRANCH[turn]}
    if turn in tf.HALF_TURNS:
        t, u = tf.gba_pair(shape, turn)
        assert gs.admissible(gba_runs(t, opts)) and gs.admissible(gba_runs(u, opts)), "replace the pair (tools/turned_spread.py --select)"


def test_case_tables_reach_what_they_are_there_for():
    turns = set(tf.TURNS)
    assert {c[2] for c in tf.POSE_CASES} == turns and {c[2] for c in tf.LBA_CASES} == turns and {c[1] for c in tf.GBA_CASES} == turns
    assert {(n, mix) for n, mix, _ in tf.POSE_CASES} == {(n, mix) for n in (10, 65) for mix in ps.MIXES}
    assert {(s, mix) for s, mix, _ in tf.LBA_CASES} == {(s, mix) for s in ((1, 1, 8), (3, 2, 64)) for mix in ls.MIXES}
    assert {s for s, _ in tf.GBA_CASES} >= set(gs.SHAPES[:3])
    # every solver in each of the three branches with trace <= 0
    assert {tf.branch_of(pose_world(*c)[0]["Tcw"][:3, :3]) for c in tf.POSE_CASES} >= {1, 2, 3}
    assert {b for c in tf.LBA_CASES for b in tf.branches_of_problem(lba_world(*c)[0]["problem"])} >= {1, 2, 3}
    assert {b for c in tf.GBA_CASES for b in tf.branches_of_problem(gba_world(*c)[0]["problem"])} >= {1, 2, 3}
    # one problem whose keyframes sit in three branches
    assert max(len(set(tf.branches_of_problem(lba_world(*c)[0]["problem"]))) for c in tf.LBA_CASES if c[2] == "d22") >= 3
    assert max(len(set(tf.branches_of_problem(gba_world(*c)[0]["problem"]))) for c in tf.GBA_CASES if c[1] == "d22") >= 3
    # a half-turn run that meets w < 0 after the quaternion product of an update, not only at the input
    assert any(pose_world(*c)[1][0]["quat_flips"]["mul"] > 0 for c in tf.POSE_CASES if c[2] in tf.HALF_TURNS)
    assert any(lba_world(*c)[1][0]["quat_flips"]["mul"] > 0 for c in tf.LBA_CASES if c[2] in tf.HALF_TURNS)
    assert any(gba_world(*c)[2][0]["quat_flips"]["mul"] > 0 for c in tf.GBA_CASES if c[1] in tf.HALF_TURNS)


def test_turning_keeps_the_camera_frame():
    """the turned scene is the same geometry: points in the camera frame move by float rounding only, measurements not at all"""
    for turn, G in tf.TURNS.items():
        u = tf.pose_case(65, "mixed", None, 0)
        t = tf.turn_pose_scene(u, G)
        cam = lambda sc: sc["obs"]["Xw"].astype(np.float64) @ sc["Tcw"][:3, :3].astype(np.float64).T + sc["Tcw"][:3, 3].astype(np.float64)
        assert np.abs(cam(t) - cam(u)).max() < 64 * 2.0 ** -24 * np.abs(cam(u)).max(), turn
        assert all(t["obs"][k] is u["obs"][k] for k in ("x", "y", "u_right", "inv_sigma2", "has_point")) and t["gross"] is u["gross"]
        u = tf.lba_case((3, 2, 64), "mixed", None, 0)
        t = tf.turn_problem(u, G)
        assert all(t["problem"][k] is u["problem"][k] for k in u["problem"] if k not in ("Tcw", "Xw"))
        assert t["gross"] is u["gross"] and t["plant"] is u["plant"] and t["behind"] is u["behind"]
        # there and back is two products of three terms each in double: 16 ulp of the largest magnitude is above their roundings
        assert np.abs(tf.turn_back_pose(t["truth_pose"], G) - u["truth_pose"])[:, :, :3].max() <= 16 * ULP_OF_ONE
        assert (tf.turn_back_pose(t["truth_pose"], G)[:, :, 3] == u["truth_pose"][:, :, 3]).all()
        assert np.abs(tf.turn_back_points(t["truth_X"], G) - u["truth_X"]).max() <= 16 * ULP_OF_ONE * np.abs(u["truth_X"]).max()
        if turn in tf.HALF_TURNS:                                          # exact: nothing but signs
            assert np.abs(t["problem"]["Tcw"]).tobytes() == np.abs(u["problem"]["Tcw"]).tobytes()
            assert np.abs(t["problem"]["Xw"]).tobytes() == np.abs(u["problem"]["Xw"]).tobytes()


# ---------------------------------------------------------------- the exact rotations

def test_exact_rotations_take_their_branch():
    names = [name for name, _, _, _ in tf.EXACT_ROTATIONS]
    assert len(set(names)) == len(names) and len(names) >= tf.N_EXACT_TABLE + 16
    per = {}
    for name, M, branch, sign in tf.EXACT_ROTATIONS:
        assert M.dtype == np.float32 and tf.branch_of(M) == branch, name
        raw = pm.quat_from_matrix(M.astype(np.float64))
        assert np.isfinite(raw).all() and (np.sign(raw[3]) == sign or (sign == 0 and raw[3] == 0.0)), (name, raw)
        if sign == 0:
            assert not np.signbit(raw[3]), name                                # +0: no flip
        if name.startswith("rand"):
            per.setdefault(branch, []).append(sign)
    for branch in (0, 1, 2, 3):
        assert len(per[branch]) >= 4
    for branch in (1, 2, 3):
        assert {+1, -1} <= set(per[branch])
    # the permutations have a trace of exactly zero, which is not > 0; the ties resolve to the FIRST of two equal largest entries
    for name, M, _, _ in tf.EXACT_ROTATIONS[:2]:
        assert float(np.trace(M.astype(np.float64))) == 0.0, name
    d = {name: np.diag(M) for name, M, _, _ in tf.EXACT_ROTATIONS}
    assert d["tie_01"][0] == d["tie_01"][1] > d["tie_01"][2] and d["tie_12"][1] == d["tie_12"][2] > d["tie_12"][0]
    assert d["tie_02"][0] == d["tie_02"][2] > d["tie_02"][1]


def test_exact_rotations_survive_the_round_trip():
    for name, M, _, _ in tf.EXACT_ROTATIONS[:tf.N_EXACT_TABLE]:
        R = round_trip(M)
        d = float(np.abs(R - M.astype(np.float64)).max())
        print(f"{name}: round trip off by {d:.3e}")
        assert np.isfinite(R).all() and d <= ULP_OF_ONE, name
    # a rotation rounded to float is orthonormal to 2^-24 per entry only; the conversion normalises, and what comes back is the nearest
    # rotation up to a few of those roundings: 32 x 2^-24 is a wide margin above them and 5 orders below a wrong sign (an entry of 0.1 or more)
    for name, M, _, _ in tf.EXACT_ROTATIONS[tf.N_EXACT_TABLE:]:
        R = round_trip(M)
        assert np.isfinite(R).all() and float(np.abs(R - M.astype(np.float64)).max()) <= 32 * 2.0 ** -24, name
        assert abs(np.linalg.det(R) - 1.0) < 1e-14, name


# ---------------------------------------------------------------- the mutations

def _pose_out(r):
    return b"".join(np.asarray(r[k]).tobytes() for k in ("pose", "Tcw", "outlier", "chi2", "n_bad", "iterations", "rounds", "ret"))


def _ba_out(r, keys):
    return b"".join(np.asarray(r[k]).tobytes() for k in ("pose", "point", "Tcw", "Xw", "chi2", "iterations", "trials") + keys)


def test_existing_pose_scenes_cannot_see_a_wrong_branch():
    for n, mix, sc in ps.all_scenes():
        base = pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], "asc")
        assert tf.branch_of(sc["Tcw"][:3, :3]) == 0
        for m in BRANCH_MUTATIONS:
            with pm.quat_mutation(m):
                assert _pose_out(pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], "asc")) == _pose_out(base), (n, mix, m)


def test_existing_lba_scenes_cannot_see_a_wrong_branch():
    for tag, sc in ls.all_scenes():
        base = lm.optimize(sc["problem"], "asc")
        assert set(tf.branches_of_problem(sc["problem"])) == {0}
        for m in BRANCH_MUTATIONS:
            with pm.quat_mutation(m):
                assert _ba_out(lm.optimize(sc["problem"], "asc"), ("edge_flags",)) == _ba_out(base, ("edge_flags",)), (tag, m)


def test_existing_gba_scenes_cannot_see_a_wrong_branch():
    for tag in gs.all_tags(big=False):
        sc, opts = gs.case(tag)
        base = gm.optimize(sc["problem"], order="asc", **opts)
        assert set(tf.branches_of_problem(sc["problem"])) == {0}
        for m in BRANCH_MUTATIONS:
            with pm.quat_mutation(m):
                assert _ba_out(gm.optimize(sc["problem"], order="asc", **opts), ("point_included",)) == _ba_out(base, ("point_included",)), (tag, m)


def _seen(base, run, diff, branches, bound, tag):
    """every branch mutation moves the outputs by more than 16 x the bound where the scene's start poses use the branch, and by nothing where
    they do not"""
    for b in (1, 2, 3):
        with pm.quat_mutation(f"quat_branch{b}"), np.errstate(all="ignore"):
            mut = run()
        d = finite(diff(base, mut))
        if b in branches:
            print(f"{tag}: quat_branch{b} changes the outputs by {d:.3e} (16 x bound {16 * max(bound.values()):.3e})")
            assert d > 16 * max(bound.values()), (tag, b)
        else:
            assert d == 0.0, (tag, b)


@pytest.mark.parametrize("n,mix,turn", tf.POSE_CASES, ids=[tf.pose_tag(*c) for c in tf.POSE_CASES])
def test_turned_pose_scene_sees_a_wrong_branch(n, mix, turn):
    sc, rs = pose_world(n, mix, turn)
    _seen(rs[0], lambda: pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], "asc"), pose_out_diff, {tf.branch_of(sc["Tcw"][:3, :3])}, POSE_BOUND,
          tf.pose_tag(n, mix, turn))


@pytest.mark.parametrize("shape,mix,turn", tf.LBA_CASES, ids=[tf.lba_tag(*c) for c in tf.LBA_CASES])
def test_turned_lba_scene_sees_a_wrong_branch(shape, mix, turn):
    sc, rs = lba_world(shape, mix, turn)
    _seen(rs[0], lambda: lm.optimize(sc["problem"], "asc"), out_diff, set(tf.branches_of_problem(sc["problem"])), LBA_BOUND,
          tf.lba_tag(shape, mix, turn))


@pytest.mark.parametrize("shape,turn", tf.GBA_CASES, ids=[tf.gba_tag(*c) for c in tf.GBA_CASES])
def test_turned_gba_scene_sees_a_wrong_branch(shape, turn):
    sc, opts, rs = gba_world(shape, turn)
    _seen(rs[0], lambda: gm.optimize(sc["problem"], order="asc", **opts), out_diff, set(tf.branches_of_problem(sc["problem"])), GBA_BOUND,
          tf.gba_tag(shape, turn))


def test_tie_rule_shows_in_the_exact_layer():
    """>= in the comparisons of the diagonal picks the LATER of two equal entries: another branch, another rounding, other bytes"""
    changed = []
    for name, M, _, _ in tf.EXACT_ROTATIONS:
        plain = round_trip(M)
        with pm.quat_mutation("quat_tie_ge"):
            if round_trip(M).tobytes() != plain.tobytes():
                changed.append(name)
    assert set(changed) & set(tf.TIES), changed
    assert not [n for n in changed if n.startswith("rand")]                 # no tie, no change


def test_the_sign_flip_is_exercised_and_not_observable():
    """q and -q are one rotation, and quat_rotate, quat_to_matrix and the quaternion product are even or bilinear in q: without the flip the
    models give the same outputs up to rounding, so nothing here or on the device pins the flip itself.  What the turned scenes pin is
    that the code around it (the negation of all four components, the normalisation behind it) is right where w < 0 occurs.  The runs
    without the flip meet w < 0 at other places than the plain ones (the counters differ): the mutation did act."""
    n, mix, turn = next(c for c in tf.POSE_CASES if c[2] in tf.HALF_TURNS and pose_world(*c)[1][0]["quat_flips"]["mul"] > 0)
    sc, rs = pose_world(n, mix, turn)
    with pm.quat_mutation("quat_no_flip"):
        mut = pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], "asc")
    assert mut["quat_flips"] != rs[0]["quat_flips"] and pose_out_diff(rs[0], mut) <= max(POSE_SPREAD_POSE, POSE_SPREAD_CHI2)
    shape, mix, turn = next(c for c in tf.LBA_CASES if c[2] in tf.HALF_TURNS and lba_world(*c)[1][0]["quat_flips"]["mul"] > 0)
    sc, rs = lba_world(shape, mix, turn)
    with pm.quat_mutation("quat_no_flip"):
        mut = lm.optimize(sc["problem"], "asc")
    assert mut["quat_flips"] != rs[0]["quat_flips"] and out_diff(rs[0], mut) <= max(LBA_SPREAD_POSE, LBA_SPREAD_POINT, LBA_SPREAD_CHI2)
    shape, turn = next(c for c in tf.GBA_CASES if c[1] in tf.HALF_TURNS and gba_world(*c)[2][0]["quat_flips"]["mul"] > 0)
    sc, opts, rs = gba_world(shape, turn)
    with pm.quat_mutation("quat_no_flip"):
        mut = gm.optimize(sc["problem"], order="asc", **opts)
    assert mut["quat_flips"] != rs[0]["quat_flips"] and out_diff(rs[0], mut) <= max(GBA_SPREAD_POSE, GBA_SPREAD_POINT, GBA_SPREAD_CHI2)
    assert math.isfinite(out_diff(rs[0], mut))
