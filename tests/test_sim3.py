"""orbx_sim3_hypotheses / orbx_sim3_hypotheses_batch (k_sim3) against tests/sim3_model.py, BIT FOR BIT and without a tolerance: n_inliers,
every mask word and the bit patterns of srt.  Each thread's arithmetic is fixed by the contract of include/orbx.h and the count is an exact
integer sum.  The jobs (tests/sim3_scene.py) hold n in {3, 20, 63, 64, 65, 257} and n_hyp in {1, 5, 63, 64, 65, 300} -- below, at and above
one mask word and one workgroup of four waves -- in batches of 1, 3 and 16 with both fix_scale values in one batch."""
import ctypes as C

import numpy as np
import pytest

import sim3_model as sm
import sim3_scene as sc

GUARD = 0xA5


def _diff(got, exp, n):
    (ni, srt, bits), (eni, esrt, ebits) = got, exp
    if ni.tobytes() != eni.tobytes():
        k = int(np.nonzero(ni != eni)[0][0])
        return f"hypothesis {k}: n_inliers {ni[k]} != {eni[k]}"
    if srt.tobytes() != esrt.tobytes():
        k = int(np.nonzero((srt.view(np.uint32) != esrt.view(np.uint32)).any(1))[0][0])
        return f"hypothesis {k}: srt {srt[k]} != {esrt[k]}"
    if bits.tobytes() != ebits.tobytes():
        k = int(np.nonzero((bits != ebits).any(1))[0][0])
        return f"hypothesis {k}: mask {bits[k]} != {ebits[k]}"
    if n % 64 and (bits[:, -1] >> np.uint64(n % 64)).any():
        return "mask bits >= n are set"
    if (np.array([bin(int(w)).count("1") for w in bits.reshape(-1)]).reshape(bits.shape).sum(1) != ni).any():
        return "n_inliers is not the number of mask bits"
    return None


def _guarded_call(pkg, jobs, batch):
    """the ABI call with every output array inside a larger block of guard bytes -> [(n_inliers, srt, bits)], asserting the guards"""
    ox, L = pkg.orbx, pkg.lib()
    arr = (ox.Sim3Job * len(jobs))()
    keep, blocks = [], []
    for i, j in enumerate(jobs):
        J, k, out = ox._sim3_job(j, "test")
        mine = []
        for name, a in zip(("n_inliers", "srt", "inlier_bits"), out):
            blk = np.full(a.nbytes + 128, GUARD, np.uint8)
            setattr(J, name, blk.ctypes.data + 64)
            mine.append((blk, a))
        arr[i] = J
        keep.append(k)
        blocks.append(mine)
    if batch:
        rc = L.orbx_sim3_hypotheses_batch(0, arr, len(jobs))
    else:
        assert len(jobs) == 1
        rc = L.orbx_sim3_hypotheses(0, C.byref(arr[0]))
    assert rc == 0, L.orbx_last_error()
    res = []
    for mine in blocks:
        outs = []
        for blk, a in mine:
            assert (blk[:64] == GUARD).all() and (blk[64 + a.nbytes:] == GUARD).all(), "written outside a job's arrays"
            outs.append(blk[64:64 + a.nbytes].view(a.dtype).reshape(a.shape).copy())
        res.append(tuple(outs))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("key", sc.keys(), ids=lambda k: f"n{k[1]}_h{k[2]}_{'fix' if k[3] else 'free'}")
def test_matches_the_model(pkg, key):
    j, exp = sc.job(*key), sc.table(*key)
    got = pkg.sim3_hypotheses(j)
    assert _diff(got, exp, key[1]) is None, _diff(got, exp, key[1])
    again = pkg.sim3_hypotheses(j)                    # the staging is reused: a second call gives the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    guarded = _guarded_call(pkg, [j], batch=False)[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, guarded))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 3, 16])
def test_batch_equals_single_calls(pkg, size):
    ks = sc.batch_keys(size)
    assert len(ks) == size and (size == 1 or len({k[3] for k in ks}) == 2)
    jobs = [sc.job(*k) for k in ks]
    got = pkg.sim3_hypotheses_batch(jobs)
    guarded = _guarded_call(pkg, jobs, batch=True)
    for k, j, g, gg in zip(ks, jobs, got, guarded):
        assert _diff(g, sc.table(*k), k[1]) is None, (k, _diff(g, sc.table(*k), k[1]))
        single = pkg.sim3_hypotheses(j)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, single)), k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, gg)), k


@pytest.mark.gpu
def test_three_unequal_jobs_in_one_batch(pkg):
    """n and n_hyp that are no multiple of the 16 bytes the staging pads to: every job's arrays lie where its own sizes put them"""
    jobs = [sc.job(400 + i, n, nh, bool(i & 1)) for i, (n, nh) in enumerate(((5, 1), (33, 3), (100, 7)))]
    got = pkg.sim3_hypotheses_batch(jobs)
    guarded = _guarded_call(pkg, jobs, batch=True)
    for j, g, gg in zip(jobs, got, guarded):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, pkg.sim3_hypotheses(j))), (len(j["X1"]), len(j["samples"]))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, gg))


@pytest.mark.gpu
def test_degenerate_hypothesis_and_special_points(pkg):
    """three coincident correspondences, a point behind camera 1 and a point with z == 0 in camera 2, for both fix_scale values"""
    for fix in (False, True):
        j = dict(sc.special_job(), fix_scale=fix)
        exp = sm.table(j)
        got = pkg.sim3_hypotheses(j)
        assert _diff(got, exp, 40) is None, _diff(got, exp, 40)
        ni, srt, bits = got
        for row in (1, 2):
            assert ni[row] == 0 and bits[row, 0] == 0 and (srt[row].view(np.uint32) == 0x7FC00000).all()
        assert not ((bits[:, 0] >> np.uint64(21)) & np.uint64(1)).any()
        assert ni[5] > 6


@pytest.mark.gpu
def test_ransac_over_the_device_table(pkg):
    """Sim3Ransac evaluates its table on the first iterate and replays the reference's loop: the same returns as the literal loop"""
    key = (105, 257, 300, False)
    j = sc.job(*key)
    for mi in (6, 150):
        r = pkg.Sim3Ransac(j, min_inliers=mi)
        seq = sm.Sequential(j, min_inliers=mi)
        for _ in range(8):
            T, more, vb, ni = r.iterate(5)
            k, more2, vb2, ni2 = seq.iterate(5)
            assert (T is None) == (k is None) and more == more2 and ni == ni2 and (vb == vb2).all()
            if k is not None:
                assert T.tobytes() == sm.T12_of(sc.table(*key)[1][k]).tobytes()
        assert r.best[0].tobytes() == seq.best[1].tobytes()
