"""orbx_bundle_adjustment (Optimizer::BundleAdjustment, reference src/Optimizer.cc:48-281) against tests/gba_model.py on the scenes of
tests/gba_scene.py.

Exact: stopped, n_active_kf, n_active_points, point_included; Tcw_out == float32(pose_out), Xw_out == float32(point_out); a keyframe
without a row (fixed, or free without an edge) is the quaternion round trip of its input; a point without edges comes back bit for bit.
iterations and trials are reported, not compared: near convergence the sign of rho is rounding noise.  pose_out, point_out and chi2 are
compared in double under a MEASURED bound:

    python tools/gba_spread.py
    SPREAD_POSE = 2.121e-12  SPREAD_POINT = 5.421e-12  SPREAD_CHI2 = 2.857e-14  (x 64: 1.357e-10, 3.469e-10, 1.828e-12)  scenes to replace: []

is the largest disagreement of the model with itself across its three summation orders over all the scenes (the 260-keyframe one sets
it), in tools/lba_spread.py's metric.  The GPU gets 64 x that spread, tests/test_lba.py's margin for the same reason: the contract leaves
the order of those sums to the implementation, and the GPU's is a fourth.  What the bound must not hide is a real error:

    python tools/gba_spread.py --mutations
    MUTATION invz_double smallest change 3.844e-08 over 10 scenes
    MUTATION float_rotation smallest change 4.156e-08 over 13 scenes
    MUTATION no_lambda_hll smallest change 9.014e-06 over 13 scenes
    MUTATION lambda_poses smallest change 9.014e-06 over 1 scenes   (all_fixed, the one scene in which a point's diagonal is the largest)
    MUTATION no_huber smallest change 2.443e-03 over 12 scenes
    MUTATION huber_5991 smallest change 2.066e-07 over 12 scenes    (LocalBundleAdjustment's delta for a monocular edge; the two small
                                                                     monocular maps carry six planted gross outliers each so that it
                                                                     shows there too: 7.4e-05 on the initial map)

and the test asserts BOUND <= SMALLEST_MUTATION / 16.  One seed was shifted (gba_scene.SEED_SHIFT): the two-keyframe monocular map with
gross outliers, whose first seeds left the model's own orders 1e-9 apart.  tests/test_gba_model.py holds every scene, the 260-keyframe
one included, to the three constants below on the model alone."""
import ctypes as C

import numpy as np
import pytest

import gba_model as gm
import gba_scene as gs
from tools.lba_spread import points_diff, poses_diff
from tools.pose_spread import chi2_diff

f32 = np.float32
SPREAD_POSE = 2.121e-12          # python tools/gba_spread.py (rounded up in the fourth digit)
SPREAD_POINT = 5.421e-12
SPREAD_CHI2 = 2.857e-14
BOUND_POSE, BOUND_POINT, BOUND_CHI2 = 64 * SPREAD_POSE, 64 * SPREAD_POINT, 64 * SPREAD_CHI2
SMALLEST_MUTATION = 3.844e-08    # python tools/gba_spread.py --mutations
assert max(BOUND_POSE, BOUND_POINT, BOUND_CHI2) <= SMALLEST_MUTATION / 16, "the bound could hide one of the listed errors"

_cache = {}


def world(tag, **kw):
    """a scene, its options and the model's answer (ascending order, with the same stop hook), computed once"""
    key = (tag, tuple(sorted(kw.items())))
    if key not in _cache:
        if ("case", tag) not in _cache:
            _cache[("case", tag)] = gs.case(tag)
        sc, opts = _cache[("case", tag)]
        _cache[key] = (sc, opts, gm.optimize(sc["problem"], order="asc", **opts, **kw))
    return _cache[key]


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def check_against_model(got, exp, pr, tag):
    dp, dx, dc = poses_diff(exp["pose"], got["pose"]), points_diff(exp["point"], got["point"]), chi2_diff(exp["chi2"], got["chi2"])
    print(f"{tag}: active kf {got['n_active_kf']} points {got['n_active_points']} iterations {got['iterations']} model {exp['iterations']} trials "
          f"{got['trials']} model {exp['trials']} chi2 {got['chi2']:.6g} lambda_init {got['lambda_init']:.4g} pose {dp:.3e} (bound {BOUND_POSE:.3e}) "
          f"point {dx:.3e} (bound {BOUND_POINT:.3e}) chi2 {dc:.3e} (bound {BOUND_CHI2:.3e})")
    assert got["stopped"] == exp["stopped"]
    assert got["n_active_kf"] == exp["n_active_kf"] and got["n_active_points"] == exp["n_active_points"]
    assert got["point_included"].tobytes() == exp["point_included"].tobytes()
    assert got["Tcw"][:, :3].tobytes() == got["pose"].astype(f32).tobytes() and got["Xw"].tobytes() == got["point"].astype(f32).tobytes()
    assert (got["Tcw"][:, 3] == np.array([0, 0, 0, 1], f32)).all()
    has_edge = np.zeros(len(pr["fixed"]), bool)
    has_edge[pr["edge_kf"]] = True
    for k in np.nonzero((np.asarray(pr["fixed"]) != 0) | ~has_edge)[0]:        # no row: the quaternion round trip of the input, exactly
        assert got["pose"][k].tobytes() == exp["pose"][k].tobytes(), k
    out = got["point_included"] == 0
    assert got["Xw"][out].tobytes() == np.asarray(pr["Xw"], f32).reshape(-1, 3)[out].tobytes()
    assert dp <= BOUND_POSE and dx <= BOUND_POINT and dc <= BOUND_CHI2


@pytest.mark.gpu
@pytest.mark.parametrize("tag", gs.all_tags())
def test_matches_the_model(pkg, tag):
    sc, opts, exp = world(tag)
    got = pkg.bundle_adjustment(sc["problem"], **opts)
    check_against_model(got, exp, sc["problem"], tag)
    if tag != gs.tag_of(gs.BIG):
        assert same_bytes(got, pkg.bundle_adjustment(sc["problem"], **opts))   # a call is byte-reproducible


@pytest.mark.gpu
def test_special_scenes_are_their_case(pkg):
    got = pkg.bundle_adjustment(world("point_without_edges")[0]["problem"])
    assert got["point_included"][5] == 0 and got["point_included"].sum() == len(got["point_included"]) - 1
    sc, opts, exp = world("kf_without_edges")
    got = pkg.bundle_adjustment(sc["problem"])
    assert got["n_active_kf"] == 2 and sc["problem"]["fixed"][1] == 0
    assert got["pose"][1].tobytes() == pkg.bundle_adjustment(sc["problem"], iterations=0)["pose"][1].tobytes()
    got = pkg.bundle_adjustment(world("no_iterations")[0]["problem"], iterations=0)
    assert (got["iterations"], got["trials"], got["stopped"], got["chi2"], got["lambda_init"]) == (0, 0, 0, 0.0, 0.0)
    assert got["Xw"].tobytes() == np.asarray(world("no_iterations")[0]["problem"]["Xw"], f32).tobytes()
    sc, opts, exp = world("not_robust")
    assert pkg.bundle_adjustment(sc["problem"], robust=True)["chi2"] < 0.9 * pkg.bundle_adjustment(sc["problem"], robust=False)["chi2"]


@pytest.mark.gpu
def test_stop_at_trial(pkg):
    tag = "11-200-mixed"
    sc, opts, full = world(tag)
    pr = sc["problem"]
    for t, stopped in ((0, 2), (2, 2), (3, 2), (full["trials"] + 1, 0)):       # 2 and 3: inside the round, between two iterations' trials
        _, _, exp = world(tag, stop_at_trial=t)
        got = pkg.bundle_adjustment(pr, stop_at_trial=t, **opts)
        assert exp["stopped"] == stopped
        check_against_model(got, exp, pr, f"{tag} stop at trial {t}")
        if stopped == 2:
            assert got["trials"] == t
        if t == 0:
            assert got["iterations"] == 0 and got["Xw"].tobytes() == np.asarray(pr["Xw"], f32).tobytes()


@pytest.mark.gpu
def test_stop_flag_up_before_the_call(pkg):
    tag = "11-200-mixed"
    sc, opts, _ = world(tag)
    _, _, exp = world(tag, stop_on_entry=True)
    flag = np.ones(1, np.uint8)
    got = pkg.bundle_adjustment(sc["problem"], stop=flag, **opts)              # no return on entry: the start estimates come back
    assert got["stopped"] == 1 and got["iterations"] == 0 and got["trials"] == 0
    check_against_model(got, exp, sc["problem"], tag + " flag up")
    assert got["pose"].tobytes() == exp["pose"].tobytes() and got["Xw"].tobytes() == np.asarray(sc["problem"]["Xw"], f32).tobytes()
    flag[0] = 0
    got = pkg.bundle_adjustment(sc["problem"], stop=flag, **opts)
    assert got["stopped"] == 0
    check_against_model(got, world(tag)[2], sc["problem"], tag + " flag down")


@pytest.mark.gpu
def test_refusals(pkg):
    L = pkg.lib()
    base = world("2-60-mono")[0]["problem"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(problem=base, null=(), drop=(), fields=None, iterations=10):
        pr, keep = pkg.orbx._lba_problem(problem, "test")
        for k, v in (fields or {}).items():
            setattr(pr, k, v)
        for k in null:
            setattr(pr, k, None)
        T = np.zeros((max(pr.n_kf, 1), 16), f32); X = np.zeros((max(pr.n_points, 1), 3), f32); inc = np.zeros(max(pr.n_points, 1), np.uint8)
        outs = dict(T=p(T), X=p(X), inc=p(inc))
        for k in drop:
            outs[k] = None
        opt = pkg.orbx.BaOptions(None, -1, iterations, 1)
        return L.orbx_bundle_adjustment(0, None if "problem" in drop else C.byref(pr), None if "opt" in drop else C.byref(opt), outs["T"], outs["X"],
                                        outs["inc"], None, None, None)

    before = L.orbx_debug_thread_contexts()
    for d in ("problem", "T", "X", "inc"):
        assert call(drop=(d,)) == -1, d
    for f in ("Tcw", "cam", "fixed", "Xw", "edge_kf", "edge_point", "x", "y", "u_right", "inv_sigma2"):
        assert call(null=(f,)) == -1, f
    assert call(iterations=-1) == -1 and "iterations" in L.orbx_last_error().decode()
    assert call(fields=dict(n_kf=0)) == -1 and call(fields=dict(n_points=-1)) == -1 and call(fields=dict(n_edges=-1)) == -1
    assert call(fields=dict(n_kf=4097)) == -2 and call(fields=dict(n_points=(1 << 20) + 1)) == -2 and call(fields=dict(n_edges=(1 << 22) + 1)) == -2
    E = len(base["edge_kf"])
    for key, val in (("edge_kf", len(base["fixed"])), ("edge_kf", -1), ("edge_point", len(base["Xw"])), ("edge_point", -1)):
        bad = dict(base); bad[key] = base[key].copy(); bad[key][E // 2] = val
        assert call(bad) == -1, (key, val)
    many = dict(base)                                                          # 2049 free keyframes
    many["Tcw"] = np.tile(base["Tcw"][:1], (2050, 1, 1)); many["cam"] = np.tile(base["cam"][:1], (2050, 1)); many["fixed"] = np.zeros(2050, np.uint8)
    many["fixed"][0] = 1
    assert call(many) == -2 and "2048" in L.orbx_last_error().decode()
    assert L.orbx_debug_thread_contexts() == before                            # refused before any device work: nothing was set up
    assert call() == 0 and call(drop=("opt",)) == 0                            # the arguments are good (opt, pose_out, point_out, report NULL)
    many["fixed"][1] = 1                                                       # 2048 free keyframes (three of them with edges) are accepted
    assert call(many) == 0
