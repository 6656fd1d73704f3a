"""The Sim3Solver model (tests/sim3_model.py) against float64, against the scenes' known similarity and against itself (the table replay
against the literal sequential loop), the truncated thresholds, the iteration count, and the refusals of orbx_sim3_hypotheses through the
Python mirror.  Nothing here needs a GPU: the refusals come before any device work."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import sim3_model as sm
import sim3_scene as sc

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# python tools/sim3_spread.py: the largest relative difference between the model's float Horn + Jacobi and the exact formulas in float64
# (numpy.linalg.eigh) on the same float inputs, over the suite's 1119 sample rows that are not near-collinear (sine of the smallest
# angle of the triangle >= 0.05 in both cameras; 11 rows, 0.97 %, are left out)
SIM3_VS_F64 = 1.042e-05
BOUND = 16 * SIM3_VS_F64


def _spread_tool():
    spec = importlib.util.spec_from_file_location("sim3_spread", os.path.join(ROOT, "tools", "sim3_spread.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_agrees_with_float64():
    """a transposed M or a wrong eigenvector is off by O(1); float Horn against float64 by the measured figure"""
    mod = _spread_tool()
    worst, count, left_out = mod.spread()
    print(f"largest relative difference {worst:.3e} over {count} hypotheses, {left_out} left out at cut-off {mod.CUT_OFF}")
    assert count > 1000
    assert left_out < 0.05 * (count + left_out)
    assert worst <= BOUND
    assert BOUND < 1e-3
    assert worst >= 0.99 * SIM3_VS_F64   # the constant is the measurement, not a looser figure


def test_noise_free_triples_recover_the_similarity():
    """three exact correspondences (up to the float rounding of the inputs) give the scene's s, R, t; R is orthonormal"""
    mod = _spread_tool()
    checked = 0
    for key in sc.keys()[1:6]:
        j = sc.job(*key)
        s, R, t = j["truth"]
        for row in j["samples"][:40]:
            P1, P2 = j["clean"][row], j["X2"][row]
            if min(sm.collinearity(P1), sm.collinearity(P2)) < mod.CUT_OFF:
                continue
            h = sm.horn(P1, P2, j["fix_scale"])
            Rm = np.array(h["R"], np.float64)
            o1 = np.linalg.norm(P1.astype(np.float64).mean(0))
            assert abs(float(h["s"]) - s) / s <= BOUND, (key, row)
            assert np.linalg.norm(Rm - R) / np.linalg.norm(R) <= BOUND, (key, row)
            assert np.linalg.norm(np.array(h["t"], np.float64) - t) / o1 <= BOUND, (key, row)
            assert np.linalg.norm(Rm @ Rm.T - np.eye(3)) <= BOUND and abs(np.linalg.det(Rm) - 1.0) <= BOUND
            checked += 1
    assert checked > 100


def test_thresholds_are_truncated():
    """mvnMaxError1/2 are vector<size_t>: (float)(size_t)(9.210 * sigma2), different from 9.210 * sigma2 at every level"""
    for k in range(8):
        sigma2 = f32(f32(1.2) ** k) * f32(f32(1.2) ** k)
        full = 9.210 * float(sigma2)
        got = sm.threshold(sigma2)
        assert got == f32(math.floor(full)) and float(got) != full and float(got) < full, k
    assert sm.threshold(1.0) == f32(9.0)
    assert [float(sm.threshold(v)) for v in sc.SIGMA2] == [9.0, 13.0, 19.0, 27.0, 39.0, 57.0, 82.0, 118.0]


def test_mirror_threshold_is_the_models(pkg):
    for v in sc.SIGMA2:
        assert pkg.sim3_max_error(v) == sm.threshold(v)


@pytest.mark.parametrize("fix_scale", [False, True])
def test_zero_imaginary_part_is_degenerate(fix_scale):
    """three coincident points: N = 0, the eigenvector is (1, 0, 0, 0) -> 0 inliers, an empty mask and NaN srt"""
    j = dict(sc.special_job(), fix_scale=fix_scale)
    for row in (1, 2):
        ni, srt, inl = sm.hypothesis(j, j["samples"][row])
        assert ni == 0 and not inl.any()
        assert (srt.view(np.uint32) == 0x7FC00000).all()


def test_z_zero_and_behind_the_camera():
    """a point with z == 0 is never an inlier; a point behind the camera projects mirrored and is tested like any other"""
    j = sc.special_job()
    ni, srt, bits = sm.table(j)
    assert ni[5] > 6 and ni[6] > 6          # the rows sampled from clean correspondences are real solutions
    for k in range(len(ni)):
        assert not sm.unpack_bits(bits[k], 40)[21]
    # the same point, mirrored through the camera centre, has the same projection in its own camera
    h = sm.horn(j["X1"][j["samples"][5]], j["X2"][j["samples"][5]], False)
    flipped = dict(j, X1=j["X1"].copy())
    flipped["X1"][20] = -j["X1"][20]
    a, b = sm.check_inliers(j, h), sm.check_inliers(flipped, h)
    assert (np.delete(a, 20) == np.delete(b, 20)).all()
    k = dict(j, X2=j["X2"].copy())
    k["X2"][21] = (0.0, 0.0, 0.0)            # 0 * inf: the error is NaN, and NaN < max is false
    assert not sm.check_inliers(k, h)[21]


def test_bits_round_trip():
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (3, 63, 64, 65, 257):
        inl = rng.uniform(size=n) < 0.5
        w = sm.pack_bits(inl)
        assert len(w) == (n + 63) // 64 and (sm.unpack_bits(w, n) == inl).all()
        assert n % 64 == 0 or int(w[-1]) >> (n % 64) == 0
        assert all((int(w[i // 64]) >> (i % 64)) & 1 == int(inl[i]) for i in range(n))


# ---- iterate: the table replay against the literal loop

def _same_state(a, b):
    assert a.iterations == b.iterations and a.best_inliers == b.best_inliers
    assert (a.best is None) == (b.best is None)
    if a.best is not None:
        assert a.best[0] == b.best[0] and a.best[1].tobytes() == b.best[1].tobytes() and (a.best[2] == b.best[2]).all()


_TABLES = {}


def _table(job):
    """the model's table of a job, computed once per sample list"""
    key = (np.asarray(job["samples"]).tobytes(), job["fix_scale"], len(job["X1"]))
    if key not in _TABLES:
        _TABLES[key] = sm.table(job)
    return _TABLES[key]


def _run_both(job, calls, mN1=None, indices1=None, mirror=None, **kw):
    """calls: a list of iterate() arguments, or "find".  -> the list of results of the sequential loop, asserted equal to the replay's
    (and to the Python mirror's Sim3Ransac over the same table, where one is given)"""
    seq = sm.Sequential(job, mN1, indices1, **kw)
    tab = _table(job)
    rep = sm.Replay(seq.N, tab, mN1, indices1, **kw)
    mir = None
    if mirror is not None:
        mir = mirror.Sim3Ransac(job, indices1, mN1, kw.get("probability", 0.99), kw.get("min_inliers", 6), kw.get("max_iterations", 300))
        mir.set_table(tab)
    out = []
    for c in calls:
        if c == "find":
            k, vb, ni = seq.find(); k2, vb2, ni2 = rep.find()
            more, more2 = None, None
        else:
            k, more, vb, ni = seq.iterate(c); k2, more2, vb2, ni2 = rep.iterate(c)
        assert k == k2 and more == more2 and ni == ni2 and (vb == vb2).all(), (c, k, k2)
        _same_state(seq, rep)
        assert seq.evaluated == seq.iterations   # the literal loop computes a hypothesis only when it reaches it
        if mir is not None:
            if c == "find":
                T, vb3, ni3 = mir.find(); more3 = None
            else:
                T, more3, vb3, ni3 = mir.iterate(c)
            assert (T is None) == (k is None) and more3 == more and ni3 == ni and (vb3 == vb).all()
            if k is not None:
                assert T.tobytes() == sm.T12_of(tab[1][k]).tobytes()
            assert mir.iterations == seq.iterations and mir.best_inliers == seq.best_inliers
            if seq.best is not None:
                assert mir.best[0].tobytes() == seq.best[1].tobytes() and mir.estimated_scale() == seq.best[1][0]
        out.append((k, more, vb, ni))
    return out, seq


@pytest.mark.parametrize("calls", [[5] * 70, [1] * 310, ["find"], [5, 1, "find"], [7, 300]], ids=["by5", "by1", "find", "mixed", "7+300"])
def test_replay_equals_the_sequential_loop(pkg, calls):
    key = (105, 257, 300, False)
    j = sc.job(*key)
    idx = np.sort(np.random.Generator(np.random.PCG64(3)).choice(400, 257, replace=False))   # mvnIndices1 into 400 matches
    for mi in (6, 20, 150, 163, 200):
        out, seq = _run_both(j, calls, mN1=400, indices1=idx, mirror=pkg, min_inliers=mi)
        returned = [o for o in out if o[0] is not None]
        for k, _, vb, ni in returned:
            assert ni > mi and vb.sum() == ni and not vb[np.setdiff1d(np.arange(400), idx)].any()
        if mi == 200:
            assert not returned and seq.iterations == min(seq.max_its, sum(c if c != "find" else 300 for c in calls))


def _rows_by_count():
    key = (105, 257, 300, False)
    j, (ni, _, _) = sc.job(*key), sc.table(*key)
    return j, ni


def _job_of_rows(j, rows):
    return dict(j, samples=np.asarray(j["samples"])[list(rows)])


def test_exactly_min_inliers_does_not_return_and_one_more_does():
    j, ni = _rows_by_count()
    c = next(int(c) for c in np.unique(ni) if c >= 6 and (ni == c + 1).any())
    lo = int(np.nonzero(ni < c)[0][0])
    a, b = int(np.nonzero(ni == c)[0][0]), int(np.nonzero(ni == c + 1)[0][0])
    out, seq = _run_both(_job_of_rows(j, [lo, a, b, lo]), [1, 1, 1, 1], min_inliers=c, max_iterations=4)
    assert [o[0] for o in out] == [None, None, 2, None]          # == min: no return; min + 1: return
    assert out[2][3] == c + 1 and out[3][1] is True              # the fourth iteration is the last: bNoMore
    assert seq.best[0] == 2


def test_a_tie_with_the_best_replaces_it():
    j, ni = _rows_by_count()
    c = next(int(c) for c in np.unique(ni) if c >= 3 and (ni == c).sum() >= 2)
    a, b = [int(i) for i in np.nonzero(ni == c)[0][:2]]
    out, seq = _run_both(_job_of_rows(j, [a, b]), [2], min_inliers=c + 5, max_iterations=2)
    assert out[0][0] is None and out[0][1] is True and seq.best[0] == 1 and seq.best_inliers == c
    out, seq = _run_both(_job_of_rows(j, [a, b]), ["find"], min_inliers=c - 1, max_iterations=2)
    assert out[0][0] == 0 and seq.iterations == 1                # find stops at the first success


def test_above_min_but_below_an_earlier_best_does_not_return():
    j, ni = _rows_by_count()
    hi = int(np.argmax(ni))
    mid = int(np.nonzero((ni > 10) & (ni < ni[hi] - 10))[0][0])
    assert ni[hi] > ni[mid] > 10
    mi = int(ni[mid]) - 3
    out, seq = _run_both(_job_of_rows(j, [hi, mid, hi]), [1, 1, 1], min_inliers=mi, max_iterations=3)
    assert [o[0] for o in out] == [0, None, 2]                    # mid > min but < best: no return; a tie with the best returns
    assert seq.best[0] == 2


def test_fewer_correspondences_than_min_inliers():
    j = sc.job(101, 20, 5, True)
    out, seq = _run_both(j, [5, "find"], min_inliers=21, max_iterations=5)
    assert out[0][0] is None and out[0][1] is True and out[0][3] == 0 and not out[0][2].any()
    assert seq.iterations == 0 and seq.evaluated == 0 and seq.max_its == 1


def test_min_inliers_equal_to_n_gives_one_iteration():
    j = sc.job(101, 20, 5, True)
    out, seq = _run_both(j, [5, 5], min_inliers=20)
    assert seq.max_its == 1 and seq.iterations == 1
    assert out[0][1] is True and out[1][1] is True and out[0][0] is None


def test_set_ransac_parameters_resets_the_iterations_only(pkg):
    j, ni = _rows_by_count()
    seq = sm.Sequential(j, min_inliers=165)
    seq.iterate(10)
    best = seq.best_inliers
    assert seq.iterations == 10 and best > 0
    seq.set_ransac_parameters(0.99, 165, 300)
    assert seq.iterations == 0 and seq.best_inliers == best      # mnBestInliers persists
    mir = pkg.Sim3Ransac(j, min_inliers=165)
    mir.set_table(sc.table(105, 257, 300, False))
    mir.iterate(10)
    mir.set_ransac_parameters(0.99, 165, 300)
    assert mir.iterations == 0 and mir.best_inliers == best and mir.table is None   # a later SetRansacParameters invalidates the table


def test_iteration_count(pkg):
    """SetRansacParameters' ceil(log(1 - p) / log(1 - eps^3)) and its clamp, (0.99, 20, 300)"""
    for N in (20, 21, 40, 100, 400):
        if N == 20:
            exp = 1
        else:
            eps = float(f32(20) / f32(N))
            exp = max(1, min(int(math.ceil(math.log(1 - 0.99) / math.log(1 - math.pow(eps, 3)))), 300))
        assert sm.ransac_iterations(0.99, 20, 300, N) == exp, N
        r = pkg.Sim3Ransac(dict(X1=np.zeros((N, 3), f32), samples=np.zeros((0, 3), np.int32)), probability=0.99, min_inliers=20, max_iterations=300)
        assert r.max_its == exp, N
    assert [sm.ransac_iterations(0.99, 20, 300, N) for N in (20, 21, 40, 100, 400)] == [1, 3, 35, 300, 300]
    assert sm.ransac_iterations(0.99, 20, 300, 10) == 1 and sm.ransac_iterations(0.99, 6, 300, 0) == 1


# ---- refusals

def _abi_job(pkg, j):
    return pkg.orbx._sim3_job(j, "t")


def test_refusals(pkg):
    """ORBX_E_INVALID / ORBX_E_CAPACITY before any device work: no GPU is needed to be refused"""
    j = sc.job(101, 20, 5, True)

    def refused(code=-1, word=None, batch=None, **over):
        with pytest.raises(pkg.OrbxError) as ei:
            if batch is not None:
                pkg.sim3_hypotheses_batch(batch)
            else:
                pkg.sim3_hypotheses(dict(j, **over))
        assert ei.value.code == code, str(ei.value)
        assert word is None or word in str(ei.value), str(ei.value)

    two = {k: j[k][:2] for k in ("X1", "X2", "max_err1", "max_err2")}
    refused(word="n = 2", samples=[[0, 1, 0]], **two)                       # n outside [3, 65535]
    big = dict(X1=np.ones((65536, 3), f32), X2=np.ones((65536, 3), f32), max_err1=np.ones(65536, f32), max_err2=np.ones(65536, f32))
    refused(word="n = 65536", **big)
    refused(word="n_hyp", samples=np.zeros((0, 3), np.int32))                # n_hyp outside [1, 1024]
    refused(word="n_hyp", samples=np.tile(np.array([[0, 1, 2]], np.int32), (1025, 1)))
    for bad in ([20, 1, 2], [0, -1, 2], [0, 1, 20]):                          # a sample index outside [0, n)
        sa = j["samples"].copy(); sa[4] = bad
        refused(word="outside", samples=sa)
    for bad in ([3, 3, 5], [3, 5, 3], [5, 3, 3]):                             # two equal indices in a row
        sa = j["samples"].copy(); sa[2] = bad
        refused(word="equal", samples=sa)
    refused(batch=[])                                                        # njobs outside [1, 64]
    refused(batch=[j] * 65)
    sa = j["samples"].copy(); sa[0] = (1, 1, 2)
    refused(word="job 2", batch=[j, j, dict(j, samples=sa)])                 # any refusal of the single call in any job
    # more than 2^22 mask words in all: 5 jobs of 1024 hypotheses x 1024 words
    n = 65535
    wide = dict(X1=np.ones((n, 3), f32), X2=np.ones((n, 3), f32), max_err1=np.ones(n, f32), max_err2=np.ones(n, f32), K1=j["K1"], K2=j["K2"],
                fix_scale=False, samples=np.tile(np.array([[0, 1, 2]], np.int32), (1024, 1)))
    refused(code=-2, word="mask words", batch=[wide] * 5)
    # NULL arguments, on the ABI itself
    L, ox = pkg.lib(), pkg.orbx
    assert L.orbx_sim3_hypotheses(0, None) == -1
    assert L.orbx_sim3_hypotheses_batch(0, None, 1) == -1
    for name in ("X1", "X2", "max_err1", "max_err2", "samples", "n_inliers", "srt", "inlier_bits"):
        J, keep, out = _abi_job(pkg, j)
        setattr(J, name, None)
        assert L.orbx_sim3_hypotheses(0, C.byref(J)) == -1, name
        J0, keep0, out0 = _abi_job(pkg, j)
        arr = (ox.Sim3Job * 2)(J0, J)
        assert L.orbx_sim3_hypotheses_batch(0, arr, 2) == -1, name
    J, keep, out = _abi_job(pkg, j)
    assert L.orbx_sim3_hypotheses_batch(0, C.byref(J), 0) == -1 and L.orbx_sim3_hypotheses_batch(0, C.byref(J), 65) == -1
