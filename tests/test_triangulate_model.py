"""The triangulation model (tests/triangulate_model.py) against itself and against numpy, and the refusals of orbx_triangulate_pairs
through the Python mirror.  Nothing here needs a GPU: the refusals come before any device work."""
import copy

import numpy as np
import pytest

import triangulate_model as tm
import triangulate_scene as ts

# python tools/tri_spread.py: the largest relative difference between the model's float Jacobi and a float64 numpy.linalg.svd of the same
# float A over the suite's accepted triangulations (2351 of them, smallest parallax 2.24 degrees)
JACOBI_VS_SVD = 1.021e-06


def test_the_two_order_rules_agree():
    """the literal sequential loop (flags updated neighbour by neighbour) == test everything, the first neighbour wins"""
    superseded = 0
    for s, (status, x3d, n_new) in ts.suite():
        st2, x2, n2 = tm.sequential(s)
        assert status.tobytes() == st2.tobytes() and x3d.tobytes() == x2.tobytes() and n_new == n2, s["name"]
        created = [int(a) for i in range(len(s["k2s"])) for a, st in zip(s["pairs"][i, 0:2 * s["npairs"][i]:2], status[i]) if st <= 2]
        assert len(created) == len(set(created)), s["name"]   # no feature of keyframe 1 gets two points
        superseded += int(np.sum(status >= 32))
    assert superseded > 100


def test_jacobi_agrees_with_a_double_svd():
    """a wrong column or a transposed A is off by O(1); float Jacobi against a double SVD by the measured figure"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("tri_spread", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tri_spread.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    worst, count, min_parallax = mod.spread()
    print(f"largest relative difference {worst:.3e} over {count} triangulations, smallest parallax {min_parallax:.3f} deg")
    assert count > 1000 and min_parallax >= 1.0
    assert worst <= 16 * JACOBI_VS_SVD
    assert 16 * JACOBI_VS_SVD < 1e-3
    assert worst >= 0.99 * JACOBI_VS_SVD   # the constant is the measurement, not a looser figure


def test_stereo_cosine_is_the_double_angle():
    """(d^2 - h^2) / (d^2 + h^2) is cos(2 atan2(h, d)), for a negative depth too"""
    for mb, d in ((0.08, 2.0), (0.54, 35.0), (0.08, -2.0), (0.1, 0.05)):
        ref = np.cos(2 * np.arctan2(np.float32(mb) / np.float32(2), np.float32(d)))
        assert abs(float(tm.stereo_cos(mb, d)) - float(ref)) <= 2 ** -23


def _call(pkg, s, **over):
    a = dict(k1=s["k1"], v1=s["v1"], k2s=s["k2s"], v2s=s["v2s"], pairs=s["pairs"], npairs=s["npairs"], sf=s["sf"], sigma2=s["sigma2"])
    a.update(over)
    return pkg.triangulate_pairs(a["k1"], a["v1"], a["k2s"], a["v2s"], a["pairs"], a["npairs"], a["sf"], a["sigma2"], s["ratio_factor"])


def test_refusals(pkg):
    """ORBX_E_INVALID / ORBX_E_CAPACITY before any device work: no GPU is needed to be refused"""
    s = next(sc for sc, _ in ts.suite() if sc["name"] == "stereo_stereo")

    def refused(code=-1, word=None, **over):
        with pytest.raises(pkg.OrbxError) as ei:
            _call(pkg, s, **over)
        assert ei.value.code == code, str(ei.value)
        assert word is None or word in str(ei.value), str(ei.value)

    n2, cap = len(s["k2s"]), s["cap"]
    refused(k2s=[], v2s=[])                                                                        # n2 outside [1, 64]
    refused(k2s=[s["k2s"][0]] * 65, v2s=[s["v2s"][0]] * 65, pairs=np.zeros((65, 2), np.int32), npairs=np.zeros(65, np.int32))
    np_ = s["npairs"].copy(); np_[1] = cap + 1
    refused(word="npairs", npairs=np_)
    np_[1] = -1
    refused(word="npairs", npairs=np_)
    for col, bad in ((0, -1), (0, ts.N1), (1, -1), (1, ts.N1)):                                    # a pair index outside its keyframe
        pr = s["pairs"].copy(); pr[n2 - 1, 2 * (s["npairs"][n2 - 1] - 1) + col] = bad
        refused(word="outside the keyframes", pairs=pr)
    refused(sf=np.ones(17, np.float32), sigma2=np.ones(17, np.float32))                            # nlevels outside [1, 16]
    refused(sf=np.ones(0, np.float32), sigma2=np.ones(0, np.float32))
    top = int(max(s["k1"]["octave"][s["pairs"][0, 0:2 * s["npairs"][0]:2]].max(), 1))
    refused(word="octave", sf=s["sf"][:top], sigma2=s["sigma2"][:top])                             # an octave outside [0, nlevels)
    k = copy.copy(s["k1"]); k["octave"] = s["k1"]["octave"].copy(); k["octave"][s["pairs"][0, 0]] = -1
    refused(word="octave", k1=k)
    k = copy.copy(s["k1"]); k["depth"] = None                                                      # stereo features, no depth
    refused(word="depth", k1=k)
    k = copy.copy(s["k1"]); k["raw_x"] = s["k1"]["x"]                                              # one raw array only
    refused(k1=k)
    # NULL arguments and cap < 1, on the ABI itself
    L, o = pkg.lib(), pkg.orbx
    f1, keep1 = o._tri_feats(s["k1"], "t")
    fs = [o._tri_feats(k2, "t") for k2 in s["k2s"]]
    import ctypes as C
    ptrs = (C.POINTER(o.TriFeats) * n2)(*[C.pointer(f[0]) for f in fs])
    views = (o.TriView * n2)(*[o._tri_view(v, "t") for v in s["v2s"]])
    v1 = o._tri_view(s["v1"], "t")
    st = np.zeros((n2, cap), np.uint8); x = np.zeros((n2, cap, 3), np.float32); nn = C.c_int()
    args = [0, C.byref(f1), C.byref(v1), ptrs, views, n2, o._p(s["pairs"]), cap, o._p(s["npairs"]), o._p(s["sf"]), o._p(s["sigma2"]), len(s["sf"]),
            float(s["ratio_factor"]), o._p(st), o._p(x), C.byref(nn)]
    for i in (1, 2, 3, 4, 6, 8, 9, 10, 13, 14, 15):
        a = list(args); a[i] = None
        assert L.orbx_triangulate_pairs(*a) == -1, i
    a = list(args); a[7] = 0
    assert L.orbx_triangulate_pairs(*a) == -1
    # more than 2^22 pairs in all: 64 lists of 65537 pairs of feature (0, 0)
    big = 65537
    refused(code=-2, k2s=[s["k2s"][0]] * 64, v2s=[s["v2s"][0]] * 64, pairs=np.zeros((64, 2 * big), np.int32), npairs=np.full(64, big, np.int32))
    # the resident calls refuse NULL handles the same way
    assert L.orbx_frame_set_depth(None, o._p(x), None, None) == -1
    assert L.orbx_frame_triangulate(None, C.byref(v1), None, views, n2, o._p(s["pairs"]), cap, o._p(s["npairs"]), o._p(s["sf"]), o._p(s["sigma2"]),
                                    len(s["sf"]), float(s["ratio_factor"]), o._p(st), o._p(x), C.byref(nn)) == -1
