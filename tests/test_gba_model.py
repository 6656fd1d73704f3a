"""tests/gba_model.py without a GPU: its blocked LDL^T is lba_model's byte for byte, the three summation orders take the same decisions on
every scene of tests/gba_scene.py -- the one of 260 free keyframes included, which sets the spread: about 17 s per order -- and agree
within the three constants tests/test_gba.py builds its bounds on (python tools/gba_spread.py), the scenes produce the cases they are named
for, and what is not a vertex keeps its value."""
import numpy as np
import pytest

import gba_model as gm
import gba_scene as gs
from test_gba import SPREAD_CHI2, SPREAD_POINT, SPREAD_POSE
from tools.lba_spread import out_diff, points_diff, poses_diff
from tools.pose_spread import chi2_diff

f32 = np.float32
SPREAD = max(SPREAD_POSE, SPREAD_POINT, SPREAD_CHI2)
TAGS = gs.all_tags()
_cache = {}


def world(tag):
    """a scene, its options and the model's answers in the three orders, computed once"""
    if tag not in _cache:
        sc, opts = gs.case(tag)
        _cache[tag] = (sc, opts, [gm.optimize(sc["problem"], order=o, **opts) for o in gm.ORDERS])
    return _cache[tag]


@pytest.mark.parametrize("n,width", [(1, 32), (5, 32), (31, 32), (32, 32), (33, 32), (66, 32), (100, 7), (258, 64), (300, 48)])
def test_blocked_ldlt_is_the_unblocked_one_byte_for_byte(n, width):
    rng = np.random.Generator(np.random.PCG64(100 * n + width))
    M = rng.normal(size=(n, n))
    S, b = M @ M.T + n * np.eye(n), rng.normal(size=n)
    x = gm.ldlt_solve(S, b)
    assert np.abs(S @ x - b).max() <= 1e-9 * max(np.abs(b).max(), 1.0) * n
    assert gm.ldlt_blocked(S, b, width).tobytes() == x.tobytes()


@pytest.mark.parametrize("j", [0, 3, 40, 65])
def test_blocked_ldlt_stops_at_a_pivot_that_is_not_positive(j):
    rng = np.random.Generator(np.random.PCG64(5))
    M = rng.normal(size=(66, 66))
    S, b = M @ M.T + 66 * np.eye(66), rng.normal(size=66)
    S[j, j] = -1.0
    assert gm.ldlt_solve(S, b) is None and gm.ldlt_blocked(S, b, 32) is None


def test_the_listed_shapes_are_all_there():
    shapes = [(s[0], s[1], s[2]) for s in gs.SHAPES + [gs.BIG]]
    for want in [(1, 60, "stereo"), (2, 60, "mono"), (11, 200, "mixed"), (12, 200, "mono"), (22, 400, "stereo"), (43, 600, "mixed"), (260, 900, "stereo")]:
        assert want in shapes
    assert (1, 60, "mono", 20) in gs.SHAPES and (2, 60, "mono", 20) in gs.SHAPES        # the initial map, with map creation's 20 iterations
    sc, _ = gs.case("1-60-mono")
    assert sc["problem"]["fixed"].tolist() == [1, 0] and (sc["problem"]["u_right"] < 0).all()


@pytest.mark.parametrize("tag", TAGS)
def test_orders_agree_on_every_decision(tag):
    sc, opts, rs = world(tag)
    assert gs.admissible(rs), "replace the scene (tools/gba_spread.py --select)"
    a, pr = rs[0], sc["problem"]
    dp = max(poses_diff(a["pose"], r["pose"]) for r in rs[1:])
    dx = max(points_diff(a["point"], r["point"]) for r in rs[1:])
    dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
    print(f"{tag}: self-disagreement pose {dp:.3e} (spread {SPREAD_POSE:.3e}) point {dx:.3e} ({SPREAD_POINT:.3e}) chi2 {dc:.3e} ({SPREAD_CHI2:.3e}) "
          f"decisions {a['decisions']}")
    assert dp <= SPREAD_POSE and dx <= SPREAD_POINT and dc <= SPREAD_CHI2       # what tests/test_gba.py multiplies by 64
    assert a["stopped"] == 0
    free_with_edge = np.zeros(len(pr["fixed"]), bool)
    free_with_edge[pr["edge_kf"]] = True
    free_with_edge &= pr["fixed"] == 0
    assert a["n_active_kf"] == int(free_with_edge.sum())
    assert a["n_active_points"] == len(np.unique(pr["edge_point"])) == int(a["point_included"].sum())
    if len(pr["edge_kf"]) and opts["iterations"]:
        assert a["iterations"] >= 1 and a["trials"] >= a["iterations"] and a["lambda_init"] > 0.0
    else:
        assert a["iterations"] == 0 and a["trials"] == 0 and a["chi2"] == 0.0


def test_what_is_not_a_vertex_keeps_its_value():
    sc, _, rs = world("point_without_edges")
    a, pr = rs[0], sc["problem"]
    assert a["point_included"][5] == 0 and a["point_included"].sum() == len(pr["Xw"]) - 1
    assert a["Xw"][5].tobytes() == np.asarray(pr["Xw"], f32)[5].tobytes()
    assert (a["Xw"][a["point_included"] == 1] != np.asarray(pr["Xw"], f32)[a["point_included"] == 1]).any(axis=1).all()
    sc, opts, rs = world("kf_without_edges")
    a, pr = rs[0], sc["problem"]
    start = gm.optimize(pr, iterations=0)                                   # the start estimates through the quaternion round trip
    assert pr["fixed"][1] == 0 and a["n_active_kf"] == 2
    assert a["pose"][1].tobytes() == start["pose"][1].tobytes()
    for k in (0, 2):
        assert a["pose"][k].tobytes() != start["pose"][k].tobytes()
    fixed = int(np.nonzero(pr["fixed"])[0][0])
    assert a["pose"][fixed].tobytes() == start["pose"][fixed].tobytes()


def test_special_scenes_produce_their_case():
    for tag in ("no_edges", "no_points"):
        sc, _, rs = world(tag)
        assert rs[0]["n_active_kf"] == 0 and rs[0]["n_active_points"] == 0 and rs[0]["trials"] == 0
    assert len(world("no_points")[0]["problem"]["Xw"]) == 0
    sc, _, rs = world("no_fixed")
    assert sc["problem"]["fixed"].sum() == 0 and rs[0]["n_active_kf"] == len(sc["problem"]["fixed"])
    sc, _, rs = world("all_fixed")
    assert rs[0]["n_active_kf"] == 0 and rs[0]["trials"] > 0
    sc, opts, rs = world("not_robust")
    assert not opts["robust"]
    assert gm.optimize(sc["problem"], iterations=10, robust=True)["chi2"] < 0.9 * rs[0]["chi2"]     # the kernel is what differs


def test_stop_hooks():
    sc, opts, rs = world("11-200-mixed")
    pr, full = sc["problem"], rs[0]
    on_entry = gm.optimize(pr, stop_on_entry=True, **opts)
    assert on_entry["stopped"] == 1 and on_entry["iterations"] == 0 and on_entry["trials"] == 0
    assert on_entry["pose"].tobytes() == gm.optimize(pr, iterations=0)["pose"].tobytes()
    assert on_entry["Xw"].tobytes() == np.asarray(pr["Xw"], f32).tobytes()
    mid = gm.optimize(pr, stop_at_trial=2, **opts)
    assert mid["stopped"] == 2 and mid["trials"] == 2 and mid["decisions"] == full["decisions"][:2]
    late = gm.optimize(pr, stop_at_trial=full["trials"] + 1, **opts)
    assert late["stopped"] == 0 and late["pose"].tobytes() == full["pose"].tobytes()


@pytest.mark.parametrize("mutation", gm.MUTATIONS)
def test_every_mutation_shows_in_some_scene(mutation):
    tags = {"lambda_poses": ["all_fixed"], "no_huber": ["11-200-mixed"], "huber_5991": ["1-60-mono", "2-60-mono"]}.get(mutation, ["11-200-mixed", "22-400-stereo"])
    for tag in tags:                                                        # huber_5991: on the initial map, the shape map creation calls with
        sc, opts, rs = world(tag)
        d = out_diff(rs[0], gm.optimize(sc["problem"], mutation=mutation, **opts))
        assert d > 1e3 * SPREAD, (tag, d)
