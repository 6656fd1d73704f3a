"""orbx_pnp_hypotheses / orbx_pnp_hypotheses_batch (k_pnp) against tests/pnp_model.py, BIT FOR BIT and without a tolerance: both counts,
every word of both masks and the bit patterns of both poses.  Each thread's arithmetic and the order of every sum over correspondences
are fixed by the contract of include/orbx.h.  The jobs (tests/pnp_scene.py) hold n in {4, 5, 63, 64, 65, 257} and n_hyp in {1, 4, 5, 35,
65} -- below, at and above one mask word and one reduction stride, below and above one workgroup of four waves -- with min_inliers at half
of n, so that some rows are refined and others are not (tests/test_pnp_model.py asserts that), in batches of 1, 3 and 16."""
import ctypes as C

import numpy as np
import pytest

import pnp_model as pm
import pnp_scene as sc

GUARD = 0xA5
NAMES = ("n_inliers", "Rt", "inlier_bits", "n_refined", "Rt_refined", "refined_bits")


def _diff(got, exp, n):
    for half, (cnt, rt, bits), (ecnt, ert, ebits) in (("", got[:3], exp[:3]), ("refined ", got[3:], exp[3:])):
        if cnt.tobytes() != ecnt.tobytes():
            k = int(np.nonzero(cnt != ecnt)[0][0])
            return f"hypothesis {k}: {half}count {cnt[k]} != {ecnt[k]}"
        if rt.tobytes() != ert.tobytes():
            k = int(np.nonzero((rt.view(np.uint64) != ert.view(np.uint64)).any(1))[0][0])
            return f"hypothesis {k}: {half}pose {rt[k]} != {ert[k]}"
        if bits.tobytes() != ebits.tobytes():
            k = int(np.nonzero((bits != ebits).any(1))[0][0])
            return f"hypothesis {k}: {half}mask {bits[k]} != {ebits[k]}"
        if n % 64 and (bits[:, -1] >> np.uint64(n % 64)).any():
            return f"{half}mask bits >= n are set"
        pop = np.array([bin(int(w)).count("1") for w in bits.reshape(-1)]).reshape(bits.shape).sum(1)
        if (pop != np.maximum(cnt, 0)).any():
            return f"{half}count is not the number of mask bits"
    return None


def _guarded_call(pkg, jobs, batch):
    """the ABI call with every output array inside a larger block of guard bytes -> [the six arrays], asserting the guards"""
    ox, L = pkg.orbx, pkg.lib()
    arr = (ox.PnpJob * len(jobs))()
    keep, blocks = [], []
    for i, j in enumerate(jobs):
        J, k, out = ox._pnp_job(j, "test")
        mine = []
        for name, a in zip(NAMES, out):
            blk = np.full(a.nbytes + 128, GUARD, np.uint8)
            setattr(J, name, blk.ctypes.data + 64)
            mine.append((blk, a))
        arr[i] = J
        keep.append(k)
        blocks.append(mine)
    if batch:
        rc = L.orbx_pnp_hypotheses_batch(0, arr, len(jobs))
    else:
        assert len(jobs) == 1
        rc = L.orbx_pnp_hypotheses(0, C.byref(arr[0]))
    assert rc == 0, L.orbx_last_error()
    res = []
    for mine in blocks:
        outs = []
        for blk, a in mine:
            assert (blk[:64] == GUARD).all() and (blk[64 + a.nbytes:] == GUARD).all(), "written outside a job's arrays"
            outs.append(blk[64:64 + a.nbytes].view(a.dtype).reshape(a.shape).copy())
        res.append(tuple(outs))
    return res


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("key", sc.keys(), ids=lambda k: f"n{k[1]}_h{k[2]}_m{k[3]}")
def test_matches_the_model(pkg, key):
    j, exp = sc.job(*key), sc.table(*key)
    got = pkg.pnp_hypotheses(j)
    assert _diff(got, exp, key[1]) is None, _diff(got, exp, key[1])
    assert _same(got, pkg.pnp_hypotheses(j))                 # the staging is reused: a second call gives the same bytes
    assert _same(got, _guarded_call(pkg, [j], batch=False)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 3, 16])
def test_batch_equals_single_calls(pkg, size):
    ks = sc.batch_keys(size)
    assert len(ks) == size and (size == 1 or (len({k[1] for k in ks}) > 1 and len({k[3] for k in ks}) > 1))
    jobs = [sc.job(*k) for k in ks]
    got = pkg.pnp_hypotheses_batch(jobs)
    guarded = _guarded_call(pkg, jobs, batch=True)
    for k, j, g, gg in zip(ks, jobs, got, guarded):
        assert _diff(g, sc.table(*k), k[1]) is None, (k, _diff(g, sc.table(*k), k[1]))
        assert _same(g, pkg.pnp_hypotheses(j)), k
        assert _same(g, gg), k


@pytest.mark.gpu
def test_three_unequal_jobs_in_one_batch(pkg):
    """n and n_hyp that are no multiple of the 16 bytes the staging pads to: every job's arrays lie where its own sizes put them"""
    jobs = [sc.job(500 + i, n, nh, sc.min_inliers_of(n)) for i, (n, nh) in enumerate(((5, 1), (33, 3), (100, 7)))]
    got = pkg.pnp_hypotheses_batch(jobs)
    guarded = _guarded_call(pkg, jobs, batch=True)
    for j, g, gg in zip(jobs, got, guarded):
        assert _same(g, pkg.pnp_hypotheses(j)), (len(j["P3Dw"]), len(j["samples"]))
        assert _same(g, gg)


@pytest.mark.gpu
def test_special_rows(pkg):
    """four coplanar samples, two samples with the same 3-D point, a correspondence behind the camera, one with z == 0 at a row's pose
    (to float rounding: tests/pnp_scene.py), and min_inliers > n, for which no row refines"""
    j = sc.special_job()
    exp = pm.table(j)
    got = pkg.pnp_hypotheses(j)
    assert _diff(got, exp, 40) is None, _diff(got, exp, 40)
    ni, rt, bits, nr, rtr, rbits = got
    assert nr[5] > j["min_inliers"] and nr[6] > j["min_inliers"]
    for mask in (bits, rbits):
        assert not ((mask[5:7, 0] >> np.uint64(20)) & np.uint64(1)).any()      # behind the camera
        assert not ((mask[5, 0] >> np.uint64(21)) & np.uint64(1))               # z == 0 at row 5's pose
    none = dict(j, min_inliers=41)
    got = pkg.pnp_hypotheses(none)
    assert _diff(got, pm.table(none), 40) is None
    assert (got[3] == -1).all() and not got[5].any() and (got[4].view(np.uint64) == 0x7FF8000000000000).all()
    assert got[0].tobytes() == ni.tobytes() and got[1].tobytes() == rt.tobytes() and got[2].tobytes() == bits.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_ransac_over_the_device_table(pkg, which):
    """PnPRansac evaluates mRansacMaxIts rows on its first iterate, replays the reference's loop and evaluates the rows past
    mRansacMaxIts only when the replay reaches them: the same returns as the literal loop over eight iterate(5) calls"""
    params = sc.RANSAC_PARAMS[which]
    s = sc.solver(*sc.RANSAC)
    r = pkg.PnPRansac(s)
    r.set_ransac_parameters(**params)
    seq = pm.Sequential(s, **params)
    early = 0
    for call in range(8):
        T, more, vb, ni = r.iterate(5)
        rt, more2, vb2, ni2 = seq.iterate(5)
        assert (T is None) == (rt is None) and more == more2 and ni == ni2 and (vb == vb2).all(), call
        if rt is not None:
            assert T.tobytes() == pm.Tcw_of(rt).tobytes(), call
            early += not more
        if call == 0:
            assert len(r.table[0]) == r.max_its                              # the tail is not evaluated before it is reached
    assert early >= 1 and r.iterations == seq.iterations > r.max_its
    assert r.max_its < len(r.table[0]) <= r.iterations + 5
    assert r.best_inliers == seq.best_inliers and r.best[0].tobytes() == seq.best[0].tobytes()
