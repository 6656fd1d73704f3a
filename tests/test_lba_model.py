"""tests/lba_model.py on the scenes of tests/lba_scene.py, without a GPU: every scene is admissible, the special scenes really produce their
case, the model reaches the truth on a noise-free scene, the classification flags the planted gross outliers, and the three summation
orders agree within the spread that tests/test_lba.py builds its bound on (python tools/lba_spread.py)."""
import numpy as np
import pytest

import lba_model as lm
import lba_scene as ls
from tools.lba_spread import out_diff, points_diff, poses_diff

SPREAD = 2.919e-12           # tools/lba_spread.py: the largest of SPREAD_POSE, SPREAD_POINT, SPREAD_CHI2
_cache = {}


def world(tag):
    """a scene and the model's answers in the three orders, computed once"""
    if tag not in _cache:
        sc = dict(ls.all_scenes())[tag]
        _cache[tag] = (sc, [lm.optimize(sc["problem"], o) for o in lm.ORDERS])
    return _cache[tag]


TAGS = [tag for tag, _ in ls.all_scenes()]


def test_no_shape_lost_all_its_mixes():
    for shape in ls.SHAPES:
        assert any((shape, mix) not in ls.DROPPED for mix in ls.MIXES)
    assert all(name in TAGS for name in ls.SPECIAL)


@pytest.mark.parametrize("tag", TAGS)
def test_scene_is_admissible_and_orders_agree(tag):
    sc, rs = world(tag)
    assert ls.admissible(sc, rs), "replace the scene (tools/lba_spread.py --select)"
    d = max(out_diff(rs[0], r) for r in rs[1:])
    print(f"{tag}: self-disagreement {d:.3e} (spread {SPREAD:.3e})")
    assert d <= SPREAD
    a = rs[0]
    assert a["stopped"] == 0
    assert a["Tcw"][:, :3].tobytes() == a["pose"].astype(np.float32).tobytes() and a["Xw"].tobytes() == a["point"].astype(np.float32).tobytes()


@pytest.mark.parametrize("tag", [t for t in TAGS if t not in ("no_edges", "no_points", "few_edges_near")])
def test_gross_outliers_and_the_point_behind_are_flagged(tag):
    sc, rs = world(tag)
    f = rs[0]["edge_flags"]
    assert (f[sc["gross"]] & 1).all() and (f[sc["gross"]] & 2).all()
    assert sc["behind"].any() and (f[sc["behind"]] == 3).all()          # isDepthPositive fails at both classifications
    clean = ~sc["gross"] & ~sc["behind"]
    assert (f[clean] == 0).mean() > 0.8                                   # the classification is not flagging everything


def test_special_scenes_produce_their_case():
    sc, rs = world("point_all_level1")
    a, pr = rs[0], sc["problem"]
    assert (a["edge_flags"][pr["edge_point"] == sc["plant"]["sp_point"]] & 1).all()
    assert a["n_active_points"][1] < a["n_active_points"][0]
    p = sc["plant"]["sp_point"]                                           # it keeps the estimate round 1 left it with
    assert not np.array_equal(a["point"][p], pr["Xw"][p].astype(np.float64))
    sc, rs = world("kf_all_level1")
    a, pr = rs[0], sc["problem"]
    assert (a["edge_flags"][pr["edge_kf"] == sc["plant"]["sp_kf"]] & 1).all() and not pr["fixed"][sc["plant"]["sp_kf"]]
    assert a["n_active_kf"] == [3, 2]
    sc, rs = world("single_edge")
    pr = sc["problem"]
    assert (pr["edge_point"] == sc["plant"]["sp_point"]).sum() == 1
    assert not np.array_equal(rs[0]["point"][0], pr["Xw"][0].astype(np.float64))      # it is optimised all the same
    sc, rs = world("fixed_only_point")
    pr = sc["problem"]
    assert pr["fixed"][pr["edge_kf"][pr["edge_point"] == 0]].all()
    assert not np.array_equal(rs[0]["point"][0], pr["Xw"][0].astype(np.float64))
    sc, rs = world("fixed_in_middle")
    pr = sc["problem"]
    k = int(np.nonzero(pr["fixed"])[0][0])
    assert 0 < k < len(pr["fixed"]) - 1 and not pr["fixed"][k - 1] and not pr["fixed"][k + 1]
    assert rs[0]["n_active_kf"][0] == int((pr["fixed"] == 0).sum())
    # the two scenes in which computeLambdaInit is decided by a point's diagonal: taken over the poses only it comes out different
    sc, rs = world("few_edges_near")
    a, pr = rs[0], sc["problem"]
    assert (pr["edge_kf"] == 0).sum() == 3 and not pr["fixed"][0] and pr["fixed"][1:].all() and a["n_active_kf"] == [1, 1]
    m = lm.optimize(pr, "asc", mutation="lambda_poses")
    assert m["lambda_init"][0] < 0.5 * a["lambda_init"][0] and m["lambda_init"][1] < a["lambda_init"][1]
    sc, rs = world("all_fixed")
    a, pr = rs[0], sc["problem"]
    assert pr["fixed"].all() and a["n_active_kf"] == [0, 0] and a["n_active_points"][0] == 64 and a["trials"][0] > 0 and a["lambda_init"][0] > 0
    assert not np.array_equal(a["point"][1], pr["Xw"][1].astype(np.float64))
    with np.errstate(all="ignore"):                                       # lambda = 0 leaves a two-view monocular point's Hll near singular
        assert lm.optimize(pr, "asc", mutation="lambda_poses")["lambda_init"] == [0.0, 0.0]
    for tag in ("no_edges", "no_points"):
        sc, rs = world(tag)
        a, pr = rs[0], sc["problem"]
        assert a["n_active_kf"] == [0, 0] and a["trials"] == [0, 0] and a["stopped"] == 0
        assert a["Xw"].tobytes() == np.asarray(pr["Xw"], np.float32).tobytes()


def test_fixed_keyframes_and_edgeless_points_keep_their_values():
    sc, rs = world("fixed_only_point")
    a, pr = rs[0], sc["problem"]
    for k in np.nonzero(pr["fixed"])[0]:
        q, t = lm.pose_from_Tcw(pr["Tcw"][k])
        assert np.array_equal(a["pose"][k, :, :3], lm.quat_to_matrix(q)) and np.array_equal(a["pose"][k, :, 3], t)
    sc, rs = world("no_edges")
    assert rs[0]["Xw"].tobytes() == sc["problem"]["Xw"].tobytes()


@pytest.mark.parametrize("mix", ls.MIXES)
def test_reaches_the_truth_without_noise(mix):
    """no noise, no outliers, nothing behind a camera: what is left is the float rounding of the measurements, 2^-24 x 640 pixels over a
    focal length of 500, some 1e-7 rad; the start is 1e-2 away.  1e-5 is a hundred times the first and a thousandth of the second."""
    sc = ls.scene(4242, 3, 2, 64, mix, noise=0.0, outliers=0.0, behind=False)
    a = lm.optimize(sc["problem"], "asc")
    start = np.asarray(sc["problem"]["Tcw"], np.float64)[:, :3]
    assert poses_diff(sc["truth_pose"], start) > 1e-3
    assert a["n_level1"] == 0 and a["n_erase"] == 0
    assert poses_diff(sc["truth_pose"], a["pose"]) < 1e-5
    assert points_diff(sc["truth_X"], a["point"]) < 1e-4                  # relative to the point's norm, which can be a tenth of the cloud's size


def test_stop_hook_paths():
    sc, rs = world("3-2-64-mixed")
    pr, full = sc["problem"], rs[0]
    a = lm.optimize(pr, "asc", stop_on_entry=True)
    assert a["stopped"] == 1 and "pose" not in a
    a = lm.optimize(pr, "asc", stop_at_trial=0)
    assert a["stopped"] == 2 and a["trials"] == [0, 0] and a["iterations"] == [0, 0]
    assert a["Tcw"].tobytes() == lm.optimize(pr, "desc", stop_at_trial=0)["Tcw"].tobytes()
    assert np.array_equal(a["edge_flags"] & 1, a["edge_flags"] >> 1)
    a = lm.optimize(pr, "asc", stop_at_trial=2)
    assert a["stopped"] == 2 and a["trials"] == [2, 0] and np.array_equal(a["edge_flags"] & 1, a["edge_flags"] >> 1)
    t = full["trials"][0] + 2
    a = lm.optimize(pr, "asc", stop_at_trial=t)
    assert a["stopped"] == 3 and a["trials"] == [full["trials"][0], 2]
    assert a["n_level1"] == full["n_level1"]
    a = lm.optimize(pr, "asc", stop_at_trial=sum(full["trials"]) + 1)
    assert a["stopped"] == 0 and a["pose"].tobytes() == full["pose"].tobytes()
