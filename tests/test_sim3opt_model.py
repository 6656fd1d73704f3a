"""tests/sim3opt_model.py and tests/sim3opt_scene.py on the CPU: every scene of the OptimizeSim3 GPU tests satisfies its condition
(sim3opt_scene.admissible: the model's variants agree on the discrete results and on the accept / reject path, no edge chi2 within 100 x
their disagreement of th2, the exit the scene was built for is reached), the measured spread recorded in tests/test_sim3opt.py still
holds, and every mutant of the model -- each a real error -- is told from the truth by 16 x the GPU test's bound or by the flags."""
import numpy as np
import pytest

import sim3opt_model as sm
import sim3opt_scene as ss
from tools.sim3opt_spread import s12_diff
from tools.pose_spread import chi2_diff

SPREAD_S12 = 1.243e-06           # python tools/sim3opt_spread.py (rounded up in the fourth digit); tests/test_sim3opt.py uses 64 x these
SPREAD_CHI2 = 4.283e-05
BOUND_S12 = 64 * SPREAD_S12

_cache = {}


def world(n, kind):
    if (n, kind) not in _cache:
        sc = ss.make_extra(kind) if kind in ss.EXTRA else ss.make(n, kind)
        _cache[(n, kind)] = (sc, ss.variants(sc))
    return _cache[(n, kind)]


@pytest.mark.parametrize("n,kind", ss.CASES + [(65, name) for name in ss.EXTRA])
def test_scene_is_admissible_and_within_the_recorded_spread(n, kind):
    sc, rs = world(n, kind)
    assert ss.admissible(n, ss.extra_kind(kind) if kind in ss.EXTRA else kind, sc, rs), "replace the scene: tools/sim3opt_spread.py --select"
    a = rs[0]
    assert max(s12_diff(a["S12"], r["S12"]) for r in rs[1:]) <= SPREAD_S12
    assert max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:]) <= SPREAD_CHI2
    spread, margin = ss.class_spread(rs)
    assert margin >= 100 * spread
    if kind == "stale":
        assert a["stale_used"] and a["rounds"] == 2


def test_the_scenes_reach_every_exit():
    seen = set()
    for n, kind in ss.CASES:
        sc, rs = world(n, kind)
        a = rs[0]
        seen.add((a["rounds"], a["more_iterations"], a["ret"] > 0))
        if a["rounds"] == 1 and a["n_bad"]:      # return 0 with the flags of round 1 cleared and g2oS12 untouched
            assert a["ret"] == 0 and a["S12"].tobytes() == np.asarray(sc["S12"], np.float64).tobytes()
            assert int(a["inlier"].sum()) == a["n_corr"] - a["n_bad"] and not a["estimate"].tobytes() == a["S12"].tobytes()
    assert {(0, 5, False), (1, 5, False), (1, 10, False), (2, 5, True), (2, 10, True)} <= seen
    fixes = {ss.case_flags(n, kind) for n, kind in ss.CASES}
    assert len(fixes) == 4                       # both values of fix_scale, a start scale of 1 and not 1


def test_camera_points_rule(pkg):
    """the package's helper forms P1c / P2c as the scenes do: (float)(double products, double sum), then the float add of t"""
    sc = ss.make(65, "outliers")
    w = sc["world"]
    assert pkg.sim3opt_camera_points(w["Xw1"], w["R1w"], w["t1w"]).tobytes() == sc["obs"]["P1c"].tobytes()
    assert pkg.sim3opt_camera_points(w["Xw2"], w["R2w"], w["t2w"]).tobytes() == sc["obs"]["P2c"].tobytes()
    wrong = (w["Xw1"].astype(np.float64) @ w["R1w"].astype(np.float64).T + w["t1w"].astype(np.float64)).astype(np.float32)
    assert wrong.tobytes() != sc["obs"]["P1c"].tobytes()      # one cast at the end is another rule


MUTANT_SCENES = [(65, "outliers"), (64, "outliers"), (11, "clean"), (257, "outliers"), (65, "nonunit")]


@pytest.mark.parametrize("mutant", sm.MUTANTS)
def test_mutant_is_told_from_the_truth(mutant):
    moved = []
    for n, kind in MUTANT_SCENES:
        sc, rs = world(n, kind)
        a = rs[0]
        m = sm.optimize(*ss.args(sc), mutant=mutant)
        d = s12_diff(a["S12"], m["S12"])
        flags = bool((m["inlier"] != a["inlier"]).any())
        print(f"{mutant} on {n} {kind}: S12 moves by {d:.3e} ({d / BOUND_S12:.1f} x the bound), flags differ {flags}")
        moved.append(d > 16 * BOUND_S12 or flags)
    # DESIGN.md names the one that neither the bound nor a flag reaches: both rounds descend to the same optimum wherever round 2 starts,
    # so an implementation that restarted round 2 from the input would pass every test here.  If it starts to show, move it out of here.
    # (normalise shows on the scene whose start quaternion is not a unit one, and only there.)
    assert any(moved) == (mutant != "round2_restart")


def test_the_path_threshold_is_far_below_the_spread():
    """admissible() lets the variants disagree on trials that move the estimate by less than NOISE_STEP: two orders below the spread the
    GPU bound is built from, so whichever way those trials fall is inside it"""
    assert 100 * ss.NOISE_STEP <= SPREAD_S12
