"""orbx_sim3_optimize and orbx_sim3_optimize_batch (Optimizer::OptimizeSim3, reference src/Optimizer.cc:1164-1365) against
tests/sim3opt_model.py on the scenes of tests/sim3opt_scene.py.

Exact: n_corr, rounds, n_bad, more_iterations, the return value, every flag; on a return of 0 S12_out is the input bit for bit.
iterations[] is not compared: at convergence the sign of rho is rounding noise.  S12 (as [s R | t] by tools/pose_spread.py's pose_diff,
and s) and chi2[] are compared in double under a MEASURED bound:

    python tools/sim3opt_spread.py
    SPREAD_S12 = 1.243e-06  SPREAD_CHI2 = 4.283e-05  (x 64: 7.955e-05, 2.741e-03)  scenes to replace: []

is the largest disagreement of the model with itself over all the scenes below across its variants: three summation orders, two seeded
one-ulp nudges of sin / cos / exp, and the closed-form Jacobian in place of the central difference.  The central difference multiplies a
last-bit difference in a projection by 5e8, so this noise is five orders of magnitude above PoseOptimization's; the chi2 figure comes
from the scenes with ONE correspondence, where 4 equations do not determine 7 unknowns and five iterations end wherever the noise
leaves them.  The GPU gets 64 x the spread, the margin k_pose_opt has, for the same reason: it differs from the model in several of
these at once.  Of six real errors that tests/test_sim3opt_model.py runs, five move S12 by more than 16 x the bound or turn a flag; a
round 2 restarted from the input does neither and would pass here.
The largest difference seen on an MI355X: see DESIGN.md."""
import ctypes as C

import numpy as np
import pytest

import sim3opt_model as sm
import sim3opt_scene as ss
from tools.pose_spread import chi2_diff
from tools.sim3opt_spread import s12_diff

SPREAD_S12 = 1.243e-06           # python tools/sim3opt_spread.py (rounded up in the fourth digit)
SPREAD_CHI2 = 4.283e-05
BOUND_S12 = 64 * SPREAD_S12      # 7.955e-05
BOUND_CHI2 = 64 * SPREAD_CHI2    # 2.741e-03

CASES = ss.CASES + [(65, name) for name in ss.EXTRA]
_cache = {}


def world(n, kind):
    """a scene and the model's plain answer, computed once"""
    if (n, kind) not in _cache:
        sc = ss.make_extra(kind) if kind in ss.EXTRA else ss.make(n, kind)
        _cache[(n, kind)] = (sc, sm.optimize(*ss.args(sc)))
    return _cache[(n, kind)]


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("S12", "inlier", "iterations", "chi2", "report_S12")) and \
        all(a[k] == b[k] for k in ("n_inliers", "n_corr", "rounds", "n_bad", "more_iterations"))


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind", CASES)
def test_matches_the_model(pkg, n, kind):
    sc, exp = world(n, kind)
    got = pkg.sim3_optimize(*ss.args(sc))
    ds = s12_diff(exp["S12"], got["S12"])
    dc = chi2_diff(exp["chi2"], got["chi2"])
    print(f"{n} {kind}: n_corr {got['n_corr']} rounds {got['rounds']} n_bad {got['n_bad']} more {got['more_iterations']} iterations "
          f"{list(got['iterations'])} model {exp['iterations']} ret {got['n_inliers']} S12 {ds:.3e} (bound {BOUND_S12:.3e}) chi2 {dc:.3e} "
          f"(bound {BOUND_CHI2:.3e})")
    assert (got["n_corr"], got["rounds"], got["n_bad"], got["more_iterations"]) == (exp["n_corr"], exp["rounds"], exp["n_bad"], exp["more_iterations"])
    assert got["n_inliers"] == exp["ret"]
    assert got["inlier"].tobytes() == exp["inlier"].tobytes(), np.nonzero(got["inlier"] != exp["inlier"])[0][:8]
    assert got["report_S12"].tobytes() == got["S12"].tobytes()
    if exp["ret"] == 0:
        assert got["S12"].tobytes() == np.asarray(sc["S12"], np.float64).tobytes()
    assert ds <= BOUND_S12 and dc <= BOUND_CHI2
    assert same_bytes(got, pkg.sim3_optimize(*ss.args(sc)))


def _jobs(count):
    """`count` jobs of unequal sizes; from two jobs on one that falls under 10 after round 1 among them, from three on an empty one too"""
    cases = [(65, "outliers"), (64, "starved"), (0, "clean"), (257, "clean"), (9, "outliers"), (64, "outliers"), (10, "clean"), (1, "starved"),
             (255, "outliers"), (63, "clean"), (256, "starved")]
    return [world(*cases[j % len(cases)])[0] for j in range(count)]


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 7, 33])
def test_batch_equals_the_single_calls(pkg, count):
    scs = _jobs(count)
    got = pkg.sim3_optimize_batch([ss.args(sc) for sc in scs])
    assert len(got) == count
    for j, sc in enumerate(scs):
        key = ("single", id(sc))
        if key not in _cache:
            _cache[key] = pkg.sim3_optimize(*ss.args(sc))
        assert same_bytes(got[j], _cache[key]), j


@pytest.mark.gpu
def test_three_unequal_jobs_in_one_batch(pkg):
    """sizes that are no multiple of the 16 bytes the staging pads to, an empty job between them: every job's arrays lie where its own
    sizes put them"""
    scs = [ss.scene(82000 + n, n, kind) for n, kind in ((33, "outliers"), (0, "clean"), (100, "clean"))]
    scs[1]["obs"] = {k: v[:0] for k, v in scs[1]["obs"].items()}                        # n = 0: no feature at all
    assert [len(sc["obs"]["x1"]) for sc in scs] == [52, 0, 153]
    got = pkg.sim3_optimize_batch([ss.args(sc) for sc in scs])
    assert len(got) == 3 and got[1]["n_corr"] == 0 and got[0]["n_corr"] > 10 and got[2]["n_corr"] > 10
    for j, sc in enumerate(scs):
        assert same_bytes(got[j], pkg.sim3_optimize(*ss.args(sc))), j


@pytest.mark.gpu
def test_refusals(pkg):
    L = pkg.lib()
    sc, _ = world(10, "clean")
    so, keep = pkg.orbx._sim3opt_obs(sc["obs"], "test")
    c1 = np.ascontiguousarray(sc["cam1"], np.float32); c2 = np.ascontiguousarray(sc["cam2"], np.float32)
    s = np.ascontiguousarray(sc["S12"], np.float64)
    out = np.zeros(8, np.float64); fl = np.zeros(so.n, np.uint8); ni = C.c_int()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda obs, c1_=c1, c2_=c2, s_=s, th2=10.0, out_=out, fl_=fl, ni_=ni: L.orbx_sim3_optimize(
        0, None if obs is None else C.byref(obs), None if c1_ is None else p(c1_), None if c2_ is None else p(c2_), None if s_ is None else p(s_),
        th2, 0, None if out_ is None else p(out_), None if fl_ is None else p(fl_), None if ni_ is None else C.byref(ni_), None)
    assert call(so) == 0                                                         # the arguments are good (report NULL)
    assert call(None) == -1 and call(so, c1_=None) == -1 and call(so, c2_=None) == -1 and call(so, s_=None) == -1
    assert call(so, out_=None) == -1 and call(so, fl_=None) == -1 and call(so, ni_=None) == -1
    for th2 in (0.0, -1.0, float("inf"), float("nan")):
        assert call(so, th2=th2) == -1, th2
    for field, _ in pkg.orbx.Sim3OptObs._fields_[1:]:
        bad = pkg.orbx.Sim3OptObs.from_buffer_copy(so)
        setattr(bad, field, None)
        assert call(bad) == -1, field
    for n in (-1, 65536):
        bad = pkg.orbx.Sim3OptObs.from_buffer_copy(so)
        bad.n = n
        assert call(bad) == -1, n
    jobs = (pkg.orbx.Sim3OptJob * 2)()
    for j in range(2):
        jobs[j].obs = C.pointer(so); jobs[j].cam1 = p(c1); jobs[j].cam2 = p(c2); jobs[j].S12 = p(s); jobs[j].th2 = 10.0
        jobs[j].S12_out = p(out); jobs[j].inlier = p(fl)
    assert L.orbx_sim3_optimize_batch(0, jobs, 2) == 0
    assert L.orbx_sim3_optimize_batch(0, jobs, 0) == -1 and L.orbx_sim3_optimize_batch(0, jobs, 65) == -1
    assert L.orbx_sim3_optimize_batch(0, None, 1) == -1
    jobs[1].cam2 = None
    assert L.orbx_sim3_optimize_batch(0, jobs, 2) == -1
