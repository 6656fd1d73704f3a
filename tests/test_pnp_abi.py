"""The refusals of orbx_pnp_hypotheses / orbx_pnp_hypotheses_batch, through the Python mirror and on the ABI itself.  They come before any
device work (as those of the Sim3 calls, tests/test_sim3_model.py), so nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import pnp_scene as sc

f32 = np.float32


def test_refusals(pkg):
    """ORBX_E_INVALID / ORBX_E_CAPACITY before any device work"""
    j = sc.job(212, 20, 5, 10)

    def refused(code=-1, word=None, batch=None, **over):
        with pytest.raises(pkg.OrbxError) as ei:
            if batch is not None:
                pkg.pnp_hypotheses_batch(batch)
            else:
                pkg.pnp_hypotheses(dict(j, **over))
        assert ei.value.code == code, str(ei.value)
        assert word is None or word in str(ei.value), str(ei.value)

    three = dict(P3Dw=j["P3Dw"][:3], P2D=j["P2D"][:3], max_err=j["max_err"][:3])
    refused(word="n = 3", samples=[[0, 1, 2, 0]], **three)                   # n outside [4, 65535]
    big = dict(P3Dw=np.ones((65536, 3), f32), P2D=np.ones((65536, 2), f32), max_err=np.ones(65536, f32))
    refused(word="n = 65536", **big)
    refused(word="n_hyp", samples=np.zeros((0, 4), np.int32))                # n_hyp outside [1, 1024]
    refused(word="n_hyp", samples=np.tile(np.array([[0, 1, 2, 3]], np.int32), (1025, 1)))
    refused(word="min_inliers = 3", min_inliers=3)                           # min_inliers < 4
    for bad in ([20, 1, 2, 3], [0, -1, 2, 3], [0, 1, 20, 3], [0, 1, 2, 20]):   # a sample index outside [0, n)
        sa = j["samples"].copy(); sa[4] = bad
        refused(word="outside", samples=sa)
    for bad in ([3, 3, 5, 6], [3, 5, 3, 6], [5, 3, 6, 3], [5, 6, 3, 3], [3, 5, 6, 3], [5, 3, 3, 6]):   # two equal indices in a row
        sa = j["samples"].copy(); sa[2] = bad
        refused(word="equal", samples=sa)
    refused(batch=[])                                                        # njobs outside [1, 64]
    refused(batch=[j] * 65)
    sa = j["samples"].copy(); sa[0] = (1, 1, 2, 3)
    refused(word="job 2", batch=[j, j, dict(j, samples=sa)])                 # any refusal of the single call in any job
    # more than 2^22 mask words in all, both masks counted: 3 jobs of 1024 hypotheses x 1024 words x 2
    n = 65535
    wide = dict(P3Dw=np.ones((n, 3), f32), P2D=np.ones((n, 2), f32), max_err=np.ones(n, f32), K=j["K"], min_inliers=4,
                samples=np.tile(np.array([[0, 1, 2, 3]], np.int32), (1024, 1)))
    refused(code=-2, word="mask words", batch=[wide] * 3)
    # NULL arguments, on the ABI itself
    L, ox = pkg.lib(), pkg.orbx
    assert L.orbx_pnp_hypotheses(0, None) == -1
    assert L.orbx_pnp_hypotheses_batch(0, None, 1) == -1
    for name in ("P3Dw", "P2D", "max_err", "samples", "n_inliers", "Rt", "inlier_bits", "n_refined", "Rt_refined", "refined_bits"):
        J, keep, out = ox._pnp_job(j, "t")
        setattr(J, name, None)
        assert L.orbx_pnp_hypotheses(0, C.byref(J)) == -1, name
        J0, keep0, out0 = ox._pnp_job(j, "t")
        arr = (ox.PnpJob * 2)(J0, J)
        assert L.orbx_pnp_hypotheses_batch(0, arr, 2) == -1, name
    J, keep, out = ox._pnp_job(j, "t")
    assert L.orbx_pnp_hypotheses_batch(0, C.byref(J), 0) == -1 and L.orbx_pnp_hypotheses_batch(0, C.byref(J), 65) == -1


def test_mirror_refuses_wrong_shapes(pkg):
    j = sc.job(212, 20, 5, 10)
    for over in (dict(P2D=j["P2D"][:19]), dict(max_err=j["max_err"][:19]), dict(samples=j["samples"][:, :3]), dict(K=j["K"][:3])):
        with pytest.raises(pkg.OrbxError):
            pkg.pnp_hypotheses(dict(j, **over))
