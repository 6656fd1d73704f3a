"""Seeded scenes for the global bundle adjustment tests, built by tests/lba_scene.py's generator with ONE fixed keyframe (the map's
keyframe with mnId == 0).  The generator gives a monocular scene two fixed keyframes; the second is freed again here, so that a monocular
map's scale is the free gauge it is in Optimizer::BundleAdjustment, held by the damping alone.

SHAPES are (free, points, mix, iterations).  (1, 60, mono, 20) is the initial map of Tracking::CreateInitialMapMonocular: two keyframes,
the first fixed, 20 iterations.  BIG is the smallest shape past both the 256 free keyframes and the 1536-entry LDS column of the
one-workgroup solver.  SPECIAL names the scenes that produce one case each; all_fixed (no row at all, the points alone are optimised) is
the one in which computeLambdaInit is decided by a point's diagonal.  case(tag) -> (scene, options) with options = dict(iterations=,
robust=) for gba_model.optimize and bundle_adjustment alike.  admissible(results): the condition every scene satisfies on the model."""
import numpy as np

import lba_scene as ls

SHAPES = [(1, 60, "stereo", 10), (1, 60, "mono", 20), (2, 60, "mono", 20), (11, 200, "mixed", 10), (12, 200, "mono", 10), (22, 400, "stereo", 10),
          (43, 600, "mixed", 10)]
BIG = (260, 900, "stereo", 3)
SPECIAL = ("no_edges", "no_points", "point_without_edges", "kf_without_edges", "no_fixed", "fixed_in_middle", "not_robust", "no_iterations",
           "all_fixed")
# tools/gba_spread.py --select: the first seed shift per tag whose scene is admissible (absent: 0)
SEED_SHIFT = {'1-60-mono': 8}


def tag_of(shape):
    return f"{shape[0]}-{shape[1]}-{shape[2]}"


def _drop_edges(pr, keep):
    for k in ("edge_kf", "edge_point", "x", "y", "u_right", "inv_sigma2"):
        pr[k] = pr[k][keep]


def _plant_gross(pr, seed, count):
    """gross outliers for a map too small for the generator's own (it plants one only where three good views of the point remain): one
    observation each of `count` points, not the point behind a camera, moved by 25 - 60 pixels.  They are what puts edges into Huber's
    linear part in the two- and three-keyframe monocular maps, so that the function's own delta shows there."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = len(pr["Xw"])
    for q in rng.permutation(P - 1)[:count]:
        e = int(np.nonzero(pr["edge_point"] == q)[0][-1])
        off = rng.uniform(25.0, 60.0, 2) * rng.choice([-1.0, 1.0], 2)
        pr["x"][e] += np.float32(off[0]); pr["y"][e] += np.float32(off[1])


def shape_scene(shape, shift=None):
    free, points, mix, _ = shape
    shift = SEED_SHIFT.get(tag_of(shape), 0) if shift is None else shift
    seed = 4242 + free + 5000 * shift + (1000 if mix == "mono" else 0)
    if mix == "mono":
        sc = ls.scene(seed, free - 1, 1, points, mix, max_views=5 if shape == BIG else 6)
        sc["problem"]["fixed"][-1] = 0                           # K = free + 1: keyframes 0 .. free - 1 and the last one free, one fixed
        if free <= 2:
            _plant_gross(sc["problem"], seed + 1, 6)
    else:
        sc = ls.scene(seed, free, 1, points, mix, max_views=5 if shape == BIG else 6)
    assert int((sc["problem"]["fixed"] == 0).sum()) == free and int(sc["problem"]["fixed"].sum()) == 1
    return sc


def special_scene(name, shift=None):
    shift = SEED_SHIFT.get(name, 0) if shift is None else shift
    seed = 7300 + SPECIAL.index(name) + 5000 * shift
    opts = dict(iterations=10, robust=True)
    if name == "all_fixed":
        return ls.scene(seed, 0, 5, 64, "mixed"), opts
    if name == "fixed_in_middle":
        sc = ls.scene(seed, 4, 1, 64, "mixed", special="fixed_in_middle")
        assert sc["problem"]["fixed"].tolist() == [0, 0, 1, 0, 0]
        return sc, opts
    sc = ls.scene(seed, 3, 1, 64, "mixed", special=name if name in ("no_edges", "no_points") else None)
    pr = sc["problem"]
    if name == "point_without_edges":
        _drop_edges(pr, pr["edge_point"] != 5)
    elif name == "kf_without_edges":
        _drop_edges(pr, pr["edge_kf"] != 1)
    elif name == "no_fixed":
        pr["fixed"][:] = 0
    elif name == "not_robust":
        opts["robust"] = False
    elif name == "no_iterations":
        opts["iterations"] = 0
    return sc, opts


def all_tags(big=True):
    return [tag_of(s) for s in SHAPES] + ([tag_of(BIG)] if big else []) + list(SPECIAL)


def case(tag, shift=None):
    """-> (scene, options)"""
    for s in SHAPES + [BIG]:
        if tag_of(s) == tag:
            return shape_scene(s, shift), dict(iterations=s[3], robust=True)
    return special_scene(tag, shift)


def admissible(results):
    """the model's three summation orders take the same accept / reject path and agree on every count; everything is finite"""
    a = results[0]
    for r in results:
        if r["decisions"] != a["decisions"] or r["point_included"].tobytes() != a["point_included"].tobytes():
            return False
        for k in ("stopped", "iterations", "trials", "n_active_kf", "n_active_points"):
            if r[k] != a[k]:
                return False
        if not (np.isfinite(r["pose"]).all() and np.isfinite(r["point"]).all() and np.isfinite(r["chi2"])):
            return False
    return True
