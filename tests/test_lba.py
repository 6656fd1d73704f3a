"""orbx_local_bundle_adjustment (Optimizer::LocalBundleAdjustment, reference src/Optimizer.cc:528-862) against tests/lba_model.py on the
scenes of tests/lba_scene.py.

Exact: edge_flags, n_level1, n_erase, n_active_kf, n_active_points, stopped; Tcw_out == float32(pose_out), Xw_out == float32(point_out);
a fixed keyframe's pose is the quaternion round trip of its input; a point without edges comes back bit for bit.  iterations[] and
trials[] are not compared: near convergence the sign of rho is rounding noise.  pose_out, point_out and chi2[] are compared in double
under a MEASURED bound:

    python tools/lba_spread.py
    SPREAD_POSE = 2.756e-13  SPREAD_POINT = 2.919e-12  SPREAD_CHI2 = 3.779e-13  (x 64: 1.764e-11, 1.868e-10, 2.419e-11)  scenes to replace: []

is the largest disagreement of the model with itself across its three summation orders over all the scenes, in tools/pose_spread.py's
metric: per pose entry relative to its block's largest magnitude, per point relative to the point's norm, per chi2 relative to
max(chi2, 1).  The GPU gets 64 x that spread, the project's precedent: it differs from the model by a fourth reduction tree and by sin /
cos.  What the bound must not hide is a real error:

    python tools/lba_spread.py --mutations
    MUTATION invz_double smallest change 8.985e-08 over 19 scenes
    MUTATION float_rotation smallest change 1.157e-07 over 25 scenes
    MUTATION no_lambda_hll smallest change 1.080e-04 over 25 scenes
    MUTATION reeval_level1 smallest change inf over 19 scenes      (it changes flags in 19 scenes and no estimate: the exact comparison catches it)
    MUTATION lambda_poses smallest change 1.158e-04 over 2 scenes  (few_edges_near and all_fixed, the two scenes in which a point's diagonal is
                                                                    the largest; in every other one a pose's is, and the error cannot show)

and the test asserts BOUND <= SMALLEST_MUTATION / 16."""
import ctypes as C

import numpy as np
import pytest

import lba_model as lm
import lba_scene as ls
from tools.lba_spread import points_diff, poses_diff
from tools.pose_spread import chi2_diff

f32 = np.float32
SPREAD_POSE = 2.756e-13          # python tools/lba_spread.py (rounded up in the fourth digit)
SPREAD_POINT = 2.919e-12
SPREAD_CHI2 = 3.779e-13
BOUND_POSE, BOUND_POINT, BOUND_CHI2 = 64 * SPREAD_POSE, 64 * SPREAD_POINT, 64 * SPREAD_CHI2
SMALLEST_MUTATION = 8.985e-08    # python tools/lba_spread.py --mutations
assert max(BOUND_POSE, BOUND_POINT, BOUND_CHI2) <= SMALLEST_MUTATION / 16, "the bound could hide one of the listed errors"

TAGS = [tag for tag, _ in ls.all_scenes()]
_cache = {}


def world(tag, **kw):
    """a scene and the model's answer (ascending order, with the same stop hook), computed once"""
    key = (tag, tuple(sorted(kw.items())))
    if key not in _cache:
        if "scenes" not in _cache:
            _cache["scenes"] = dict(ls.all_scenes())
        sc = _cache["scenes"][tag]
        _cache[key] = (sc, lm.optimize(sc["problem"], "asc", **kw))
    return _cache[key]


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def check_against_model(got, exp, pr, tag):
    dp, dx, dc = poses_diff(exp["pose"], got["pose"]), points_diff(exp["point"], got["point"]), chi2_diff(exp["chi2"], got["chi2"])
    print(f"{tag}: active kf {got['n_active_kf']} points {got['n_active_points']} iterations {got['iterations']} model {exp['iterations']} trials "
          f"{got['trials']} model {exp['trials']} level1 {got['n_level1']} erase {got['n_erase']} margins {exp['margin_chi2']:.2e} {exp['margin_depth']:.2e} "
          f"pose {dp:.3e} (bound {BOUND_POSE:.3e}) point {dx:.3e} (bound {BOUND_POINT:.3e}) chi2 {dc:.3e} (bound {BOUND_CHI2:.3e})")
    assert exp["margin_chi2"] >= ls.MARGIN and exp["margin_depth"] >= ls.MARGIN, "the scene has an edge within 1e-6 of a threshold: replace it"
    assert got["stopped"] == exp["stopped"]
    assert got["edge_flags"].tobytes() == exp["edge_flags"].tobytes(), np.nonzero(got["edge_flags"] != exp["edge_flags"])[0][:8]
    assert (got["n_level1"], got["n_erase"]) == (exp["n_level1"], exp["n_erase"])
    assert got["n_active_kf"] == exp["n_active_kf"] and got["n_active_points"] == exp["n_active_points"]
    assert got["Tcw"][:, :3].tobytes() == got["pose"].astype(f32).tobytes() and got["Xw"].tobytes() == got["point"].astype(f32).tobytes()
    assert (got["Tcw"][:, 3] == np.array([0, 0, 0, 1], f32)).all()
    for k in np.nonzero(pr["fixed"])[0]:                                   # the quaternion round trip of the input, exactly
        assert got["pose"][k].tobytes() == exp["pose"][k].tobytes(), k
    deg = np.bincount(pr["edge_point"], minlength=len(pr["Xw"]))
    assert got["Xw"][deg == 0].tobytes() == np.asarray(pr["Xw"], f32)[deg == 0].tobytes()
    assert dp <= BOUND_POSE and dx <= BOUND_POINT and dc <= BOUND_CHI2


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_matches_the_model(pkg, tag):
    sc, exp = world(tag)
    got = pkg.local_bundle_adjustment(sc["problem"])
    check_against_model(got, exp, sc["problem"], tag)
    assert same_bytes(got, pkg.local_bundle_adjustment(sc["problem"]))     # a call is byte-reproducible


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["3-2-64-mixed", "11-3-200-stereo"])
def test_stop_at_trial(pkg, tag):
    sc, full = world(tag)
    pr = sc["problem"]
    r1 = full["trials"][0]
    for t, stopped in ((0, 2), (2, 2), (r1 + 2, 3), (sum(full["trials"]) + 1, 0)):
        _, exp = world(tag, stop_at_trial=t)
        got = pkg.local_bundle_adjustment(pr, stop_at_trial=t)
        assert exp["stopped"] == stopped
        check_against_model(got, exp, pr, f"{tag} stop at trial {t}")
        if stopped == 2:                                                   # round 2 skipped: the final check is the same test as bit 0
            assert got["trials"] == [t, 0] and np.array_equal(got["edge_flags"] & 1, got["edge_flags"] >> 1)
        if t == 0:                                                         # the state at the start estimates
            assert got["iterations"] == [0, 0]
            assert got["Xw"].tobytes() == np.asarray(pr["Xw"], f32).tobytes()
        if stopped == 3:
            assert got["trials"][0] > 0 and got["trials"][1] > 0 and got["n_level1"] == full["n_level1"]


@pytest.mark.gpu
def test_stop_flag_up_before_the_call(pkg):
    sc, _ = world("3-2-64-mixed")
    L = pkg.lib()
    pr, keep = pkg.orbx._lba_problem(sc["problem"], "test")
    flag = np.ones(1, np.uint8)
    opt = pkg.orbx.LbaOptions(flag.ctypes.data, -1)
    T = np.full((pr.n_kf, 16), 7, f32); X = np.full((pr.n_points, 3), 7, f32); fl = np.full(pr.n_edges, 7, np.uint8)
    po = np.full((pr.n_kf, 12), 7.0); pt = np.full((pr.n_points, 3), 7.0); rep = pkg.orbx.LbaReport()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.orbx_local_bundle_adjustment(0, C.byref(pr), C.byref(opt), p(T), p(X), p(fl), p(po), p(pt), C.byref(rep)) == 0
    assert rep.stopped == 1 and list(rep.trials) == [0, 0]
    assert (T == 7).all() and (X == 7).all() and (fl == 7).all() and (po == 7).all() and (pt == 7).all()
    flag[0] = 0                                                            # the same options with the flag down: a full run
    assert L.orbx_local_bundle_adjustment(0, C.byref(pr), C.byref(opt), p(T), p(X), p(fl), p(po), p(pt), C.byref(rep)) == 0
    assert rep.stopped == 0 and fl.tobytes() == world("3-2-64-mixed")[1]["edge_flags"].tobytes()


@pytest.mark.gpu
def test_refusals(pkg):
    L = pkg.lib()
    sc, _ = world("2-2-20-mixed")
    base = sc["problem"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(problem=base, null=(), drop=(), fields=None):
        pr, keep = pkg.orbx._lba_problem(problem, "test")
        for k, v in (fields or {}).items():
            setattr(pr, k, v)
        for k in null:
            setattr(pr, k, None)
        T = np.zeros((max(pr.n_kf, 1), 16), f32); X = np.zeros((max(pr.n_points, 1), 3), f32); fl = np.zeros(max(pr.n_edges, 1), np.uint8)
        outs = dict(T=p(T), X=p(X), fl=p(fl))
        for k in drop:
            outs[k] = None
        return L.orbx_local_bundle_adjustment(0, None if "problem" in drop else C.byref(pr), None, outs["T"], outs["X"], outs["fl"], None, None, None)

    assert call() == 0                                                     # the arguments are good (opt, pose_out, point_out, report NULL)
    for d in ("problem", "T", "X", "fl"):
        assert call(drop=(d,)) == -1, d
    for f in ("Tcw", "cam", "fixed", "Xw", "edge_kf", "edge_point", "x", "y", "u_right", "inv_sigma2"):
        assert call(null=(f,)) == -1, f
    assert call(fields=dict(n_kf=0)) == -1 and call(fields=dict(n_points=-1)) == -1 and call(fields=dict(n_edges=-1)) == -1
    assert call(fields=dict(n_kf=1025)) == -2 and call(fields=dict(n_points=(1 << 20) + 1)) == -2 and call(fields=dict(n_edges=(1 << 22) + 1)) == -2
    E = len(base["edge_kf"])
    for key, val in (("edge_kf", len(base["fixed"])), ("edge_kf", -1), ("edge_point", len(base["Xw"])), ("edge_point", -1)):
        bad = dict(base); bad[key] = base[key].copy(); bad[key][E // 2] = val
        assert call(bad) == -1, (key, val)
    bad = dict(base); bad["edge_point"] = base["edge_point"].copy()        # the edges of a point not contiguous / points not ascending
    bad["edge_point"][0], bad["edge_point"][-1] = base["edge_point"][-1], base["edge_point"][0]
    assert call(bad) == -1 and "contiguous" in L.orbx_last_error().decode()
    bad = dict(base); bad["edge_kf"] = base["edge_kf"].copy()              # two edges between one point and one keyframe
    bad["edge_kf"][1] = bad["edge_kf"][0]
    assert base["edge_point"][1] == base["edge_point"][0] and call(bad) == -1 and "second edge" in L.orbx_last_error().decode()
    many = dict(base)                                                      # 257 free keyframes
    many["Tcw"] = np.tile(base["Tcw"][:1], (258, 1, 1)); many["cam"] = np.tile(base["cam"][:1], (258, 1)); many["fixed"] = np.zeros(258, np.uint8)
    many["fixed"][0] = 1
    assert call(many) == -2 and "256" in L.orbx_last_error().decode()
    many["fixed"][1] = 1                                                   # 256 of them are accepted
    assert call(many) == 0
