"""The PnPsolver model (tests/pnp_model.py) against itself -- the replay over a table whose rows are refined from their own masks against
the literal sequential loop, which refines from the best set as the reference does -- against an independent evaluation of the same EPnP
with numpy.linalg in place of the Jacobi restatements, SetRansacParameters' known answers, and the condition the device tests rest on: the
model alone finds a refined pose inside the table for every RANSAC setting they use.  Nothing here needs a GPU."""
import numpy as np
import pytest

import pnp_model as pm
import pnp_scene as sc

f32 = np.float32

# Measured here (python -m pytest tests/test_pnp_model.py -s prints them): the largest deviation of the numpy.linalg evaluation from the
# scene's true pose over the noise-free sample rows in general position, max |R - R_true| and |t - t_true| / |t_true| together, and the
# same for the refinement from all correspondences of a noise-free scene.  The model is asserted at 64 x these, the margin of pose_model /
# sim3opt_model.  Four-point EPnP is ill-conditioned (MtM has a four-dimensional null space and the three beta approximations pick among
# local solutions), so the first figure is large and its bound loose; the refinement figure is the sharp one.
CUT = 0.25                      # general position: the smallest singular value of the centred sample points, in metres
NOISE_FREE = [(900 + i, 64, 12) for i in range(4)]
LINALG_VS_TRUTH_4 = 2.480e+01   # numpy.linalg against the truth over the 31 four-point rows in general position (the model: 2.319e+01)
LINALG_VS_TRUTH_64 = 2.573e-07  # ... and for the refinement from all 64 correspondences (the model: 2.709e-07)


def _dev(R, t, truth):
    Rt, tt = truth
    return max(float(np.abs(R - Rt).max()), float(np.linalg.norm(t - tt) / np.linalg.norm(tt)))


@pytest.fixture(scope="module")
def spread():
    """-> (rows [(key, row, model deviation, linalg deviation)], refinements [(key, model deviation, linalg deviation)])"""
    rows, refs = [], []
    for key in NOISE_FREE:
        j = sc.job(*key, 32, 0.0, 0.0)
        for r, s in enumerate(j["samples"]):
            if pm.general_position(j["P3Dw"][s]) < CUT:
                continue
            R, t = pm.compute_pose(j, pm.Members(j, s, True))
            R2, t2 = pm.pose_linalg(j, s)
            rows.append((key, r, _dev(R, t, j["truth"]), _dev(R2, t2, j["truth"])))
        every = pm.Members(j, np.arange(64), False)
        R, t = pm.compute_pose(j, every)
        R2, t2 = pm.compute_pose(j, every, linalg=pm.Linalg)
        refs.append((key, _dev(R, t, j["truth"]), _dev(R2, t2, j["truth"])))
    return rows, refs


def test_model_against_numpy_linalg(spread):
    """the same EPnP with numpy.linalg.svd / lstsq / inv: both agree with the truth on noise-free scenes, the model within 64 x the
    independent evaluation's own largest deviation"""
    rows, refs = spread
    assert len(rows) >= 30
    lin4, mod4 = max(r[3] for r in rows), max(r[2] for r in rows)
    linr, modr = max(r[2] for r in refs), max(r[1] for r in refs)
    print(f"four-point rows in general position: {len(rows)}; numpy.linalg vs truth {lin4:.3e}, model vs truth {mod4:.3e}")
    print(f"refinement from 64 correspondences: numpy.linalg vs truth {linr:.3e}, model vs truth {modr:.3e}")
    assert mod4 <= 64 * LINALG_VS_TRUTH_4
    assert modr <= 64 * LINALG_VS_TRUTH_64
    assert 64 * LINALG_VS_TRUTH_64 < 1e-3   # the refinement bound means something: a wrong sum or a transposed matrix is off by O(1)
    # the sharp constant is the measurement, not a looser figure.  (The four-point figure is printed only: it is one ill-conditioned
    # row's miss, and a LAPACK build that rounds differently may miss on another row.)
    assert 0.5 * LINALG_VS_TRUTH_64 <= linr <= 2 * LINALG_VS_TRUTH_64


def test_the_lane_ordered_sum_is_a_sum():
    """Members.sum in mask form adds every member once, whatever n: against math.fsum"""
    import math
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (4, 63, 64, 65, 257):
        j = dict(P3Dw=np.zeros((n, 3), f32), P2D=np.zeros((n, 2), f32))
        mask = rng.uniform(size=n) < 0.6
        mask[0] = True
        M = pm.Members(j, np.nonzero(mask)[0], False)
        x = rng.normal(size=int(mask.sum()))
        assert abs(float(M.sum(x)) - math.fsum(x)) <= 1e-13 * np.abs(x).sum()


def test_round_robin_covers_every_pair_once():
    for n in (3, 4, 5, 12):
        seen = []
        for rnd in pm.round_robin(n):
            cols = [c for pq in rnd for c in pq]
            assert len(cols) == len(set(cols))           # the pivots of a round are disjoint
            seen += rnd
        assert sorted(seen) == [(p, q) for p in range(n) for q in range(p + 1, n)]


def test_svd_is_an_svd():
    rng = np.random.Generator(np.random.PCG64(6))
    for m, n in ((3, 3), (6, 3), (6, 4), (6, 5), (12, 12)):
        A = rng.normal(size=(m, n))
        if m == n:
            A = A @ A.T
        Ar, V, w = pm.svd(A)
        assert np.abs(np.sort(w)[::-1] - np.linalg.svd(A, compute_uv=False)).max() < 1e-12 * w.max()
        assert np.abs(A @ V - Ar).max() < 1e-12 * w.max() and np.abs(V.T @ V - np.eye(n)).max() < 1e-13
        b = rng.normal(size=m)
        assert np.abs(np.array(pm.solve(Ar, V, w, b)) - np.linalg.lstsq(A, b, rcond=None)[0]).max() < 1e-9


@pytest.mark.parametrize("N", [20, 100, 1000])
def test_set_ransac_parameters_with_relocalization_arguments(pkg, N):
    """SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) gives 35 rows, not 300"""
    assert pm.ransac_parameters(N, 0.99, 10, 300, 4, 0.5)[2] == 35
    s = sc.solver(400 + N, N, 1)
    r = pkg.PnPRansac(s)
    r.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
    assert r.max_its == 35 and r.min_inliers == max(10, N // 2)
    assert r.max_err.tobytes() == (s["sigma2"] * f32(5.991)).astype(f32).tobytes()


def test_set_ransac_parameters_known_answers(pkg):
    mi, eps, its = pm.ransac_parameters(15, 0.99, 10, 300, 4, 0.5)
    assert mi == 10 and eps == f32(10) / f32(15) and abs(float(eps) - 2 / 3) < 1e-7
    assert pm.ransac_parameters(10, 0.99, 10, 300, 4, 0.5) == (10, f32(1.0), 1)        # N == min_inliers: one row
    assert pm.ransac_parameters(9, 0.99, 10, 300, 4, 0.5)[0] == 10                     # N < min_inliers: iterate refuses
    assert pm.ransac_parameters(100, 0.99, 8, 300, 4, 0.4)[0] == 40                    # int(100 * 0.4f) truncates 40.000001
    assert pm.ransac_parameters(100, 0.99, 8, 5, 4, 0.4)[2] == 5                       # min(nIterations, maxIts)
    for N in (15, 10, 100):
        r = pkg.PnPRansac(sc.solver(500 + N, N, 1))
        r.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
        assert (r.min_inliers, r.epsilon, r.max_its) == pm.ransac_parameters(N, 0.99, 10, 300, 4, 0.5)
    r = pkg.PnPRansac(sc.solver(509, 9, 1))
    r.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
    assert r.iterate(5)[:2] == (None, True)             # N < mRansacMinInliers: bNoMore, before any device work


def _ransac_table(params):
    seed, n, rows = sc.RANSAC
    mi = pm.ransac_parameters(n, *[params[k] for k in ("probability", "min_inliers", "max_iterations", "min_set", "epsilon")])[0]
    return sc.table(seed, n, rows, mi)


@pytest.mark.parametrize("which", [0, 1])
def test_sequential_equals_the_replay_with_own_mask_refinement(which):
    """Refine reads the best set so far; the table refines every qualifying row from its own mask.  The two give the same returns, counts
    and masks at every iterate(5) -- also after an early return and past mRansacMaxIts."""
    params = sc.RANSAC_PARAMS[which]
    s = sc.solver(*sc.RANSAC)
    seq = pm.Sequential(s, **params)
    rep = pm.Replay(s, _ransac_table(params), **params)
    early = 0
    for _ in range(8):
        a, b = seq.iterate(5), rep.iterate(5)
        assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3] and (a[2] == b[2]).all()
        if a[0] is not None:
            assert a[0].tobytes() == b[0].tobytes()
            early += not a[1]
    assert seq.iterations == rep.iterations and seq.best_inliers == rep.best_inliers
    assert early >= 1 and seq.iterations > seq.max_its        # it returned early and was called again past mRansacMaxIts


@pytest.mark.parametrize("which", [0, 1])
def test_the_scenes_let_the_model_find_a_refined_pose(which):
    """the condition the device test of the RANSAC rests on: inside the table the model alone returns a refined pose with more than
    min_inliers inliers, close to the scene's pose -- no GPU test can pass by finding nothing"""
    params = sc.RANSAC_PARAMS[which]
    s = sc.solver(*sc.RANSAC)
    rep = pm.Replay(s, _ransac_table(params), **params)
    rt, no_more, vb, ni = rep.iterate(5)
    assert rt is not None and not no_more and rep.iterations <= rep.max_its
    assert ni > rep.min_inliers and vb.sum() == ni and not (vb & s["is_outlier"]).any()
    R, t = s["truth"]
    assert np.abs(rt[:9].reshape(3, 3) - R).max() < 2e-2 and np.abs(rt[9:] - t).max() < 5e-2


def test_the_device_shapes_refine_some_rows_and_not_others():
    """over the jobs of tests/test_pnp.py both kinds of row occur, and every job with more than one row and outliers has both"""
    kinds = set()
    for key in sc.keys():
        nr = sc.table(*key)[3]
        kinds |= {bool(v >= 0) for v in nr}
        if key[1] >= 63 and key[2] >= 35:
            assert (nr >= 0).any() and (nr < 0).any(), key
    assert kinds == {True, False}


def test_special_rows_of_the_model():
    j = sc.special_job()
    ni, rt, bits, nr, rtr, rbits = pm.table(j)
    assert nr.max() > j["min_inliers"]                   # the special points are tested against rows that have a solution
    assert nr[5] > j["min_inliers"]
    Rm, tm = j["row5_pose"]
    P = j["P3Dw"][21].astype(np.float64)
    assert abs(pm.dot3(Rm[2], P) + tm[2]) < 1e-5         # z == 0 at row 5's pose, to float rounding
    assert not pm.unpack_bits(bits[5], 40)[21] and not pm.unpack_bits(bits[5], 40)[20]
    none = pm.table(dict(j, min_inliers=41))             # min_inliers > n: no row refines
    assert (none[3] == -1).all() and not none[5].any() and (none[4].view(np.uint64) == 0x7FF8000000000000).all()
    assert none[0].tobytes() == ni.tobytes() and none[1].tobytes() == rt.tobytes()


def test_bits_round_trip():
    rng = np.random.Generator(np.random.PCG64(3))
    for n in (4, 63, 64, 65, 257):
        inl = rng.uniform(size=n) < 0.5
        w = pm.pack_bits(inl)
        assert len(w) == (n + 63) // 64 and (pm.unpack_bits(w, n) == inl).all()
        if n % 64:
            assert int(w[-1]) >> (n % 64) == 0
