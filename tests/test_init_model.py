"""The Initializer model (tests/init_model.py) against float64, against the scenes' known motion and against itself (the array forms
against the reference's sequential text), the acos thresholds, the degenerate rows, the mask round trip, and the refusals of the three
orbx_mono_init_* calls through the Python mirror.  Nothing here needs a GPU: the refusals come before any device work."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import init_model as im
import init_scene as sc

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# python tools/init_spread.py: the largest component by which the model's null vector (float one-sided Jacobi) differs from
# numpy.linalg.svd in float64 on the same 16 x 9 / 8 x 9 float matrix, over the suite's 1846 sample rows whose two smallest singular
# values are not closer than s8 = 0.5 * s7 (170 rows, 8.43 %, are left out); the project's margin of 64 on top
NULL_VS_F64 = 2.901e-04
NULL_BOUND = 64 * NULL_VS_F64
# the same tool: the angles between the model's R21 / t21 and the scene's motion on the noise-free twins of general and planar
ROT_VS_SCENE_DEG, T_VS_SCENE_DEG = 2.583e-02, 9.630e-04
# Residuals of noise-free matches.  The keypoints are rounded to float (half an ulp of 640 is 3.1e-5 px) and every product of the
# check is rounded once more (FLT_EPSILON * 640 = 7.6e-5 px); a well-conditioned sample row therefore leaves a few 1e-4 px, and 1e-2 px
# -- a hundredth of sigma, a few hundred roundings -- is the level below which the ROW THAT WINS must hold EVERY match.
ROUNDING_PX = 1e-2
ROUNDING_MEDIAN_PX = 1e-3   # over the rows of a table, on their own eight matches: a dozen roundings


def _spread_tool():
    spec = importlib.util.spec_from_file_location("init_spread", os.path.join(ROOT, "tools", "init_spread.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_null_vectors_agree_with_float64():
    """a transposed system or a wrong column of V is off by O(1); the float Jacobi against float64 by the measured figure"""
    mod = _spread_tool()
    worst, count, left_out = mod.null_spread()
    print(f"largest disagreement {worst:.3e} over {count} rows, {left_out} left out at ratio {mod.RATIO}")
    assert count > 1500
    assert left_out <= 0.10 * (count + left_out)          # the cap of the condition
    assert worst <= NULL_BOUND
    assert NULL_BOUND < 0.05
    assert worst >= 0.99 * NULL_VS_F64   # the constant is the measurement, not a looser figure


def _residuals(key):
    """per row of the table: the epipolar distance (F) and the transfer error (H) in pixels of every match, in float64"""
    j, tab = sc.job(*key), sc.table(*key)
    pts = im.gather(j).astype(np.float64)
    x1 = np.concatenate([pts[:, :2], np.ones((len(pts), 1))], 1)
    x2 = np.concatenate([pts[:, 2:], np.ones((len(pts), 1))], 1)
    Fm, Hm = tab[4].astype(np.float64).reshape(-1, 3, 3), tab[1].astype(np.float64).reshape(-1, 3, 3)
    line = np.einsum("hij,nj->hni", Fm, x1)
    dist = np.abs(np.einsum("hni,ni->hn", line, x2)) / np.hypot(line[..., 0], line[..., 1])
    y = np.einsum("hij,nj->hni", Hm, x1)
    transfer = np.hypot(y[..., 0] / y[..., 2] - x2[:, 0], y[..., 1] / y[..., 2] - x2[:, 1])
    return dist, transfer


def test_noise_free_samples_fit_at_rounding_level():
    for kind in ("general", "planar"):
        key = sc.MAIN[kind] + (0.0,)
        j, r = sc.job(*key), sc.result(*key)
        dist, transfer = _residuals(key)
        sa = j["samples"]
        own_f = np.array([dist[h, sa[h]].max() for h in range(len(sa))])
        print(f"{kind}: x2^T F x1 on the row's own matches: median {np.median(own_f):.3e} px; winner over all {dist[r['best_f']].max():.3e} px")
        assert np.median(own_f) <= ROUNDING_MEDIAN_PX
        assert dist[r["best_f"]].max() <= ROUNDING_PX
        if kind == "planar":
            own_h = np.array([transfer[h, sa[h]].max() for h in range(len(sa))])
            print(f"{kind}: H transfer on the row's own matches: median {np.median(own_h):.3e} px; winner over all {transfer[r['best_h']].max():.3e} px")
            assert np.median(own_h) <= ROUNDING_MEDIAN_PX
            assert transfer[r["best_h"]].max() <= ROUNDING_PX
        else:
            assert np.median(transfer) > 1.0   # no homography fits a depth-varied cloud


def test_the_model_picks_h_on_planar_and_f_on_general():
    for noise in (0.3, 0.0):
        g, p = sc.result(*sc.MAIN["general"], noise), sc.result(*sc.MAIN["planar"], noise)
        assert g["model"] == 2 and g["ok"] and g["winner"] in range(4)
        assert p["model"] == 1 and p["ok"] and p["winner"] in range(8)
        assert g["n_good"][4:].sum() == 0
    o = sc.result(*sc.MAIN["outliers"])
    assert o["model"] == 2


def test_recovered_motion_matches_the_scene():
    mod = _spread_tool()
    rot, tr, k = mod.motion_spread()
    print(f"rotation {rot:.3e} deg, translation direction {tr:.3e} deg over {k} jobs")
    assert k == 2
    assert rot <= 64 * ROT_VS_SCENE_DEG and tr <= 64 * T_VS_SCENE_DEG
    assert 64 * ROT_VS_SCENE_DEG < 5.0 and 64 * T_VS_SCENE_DEG < 5.0     # a mirrored t or a swapped R1 / R2 is off by tens of degrees
    assert rot >= 0.99 * ROT_VS_SCENE_DEG and tr >= 0.99 * T_VS_SCENE_DEG
    for key in mod.MOTION_KEYS:
        r, j = sc.result(*key), sc.job(*key)
        Rm = r["R21"].astype(np.float64)
        assert np.linalg.norm(Rm @ Rm.T - np.eye(3)) < 1e-5 and abs(np.linalg.det(Rm) - 1.0) < 1e-5
        assert abs(np.linalg.norm(r["t21"].astype(np.float64)) - 1.0) < 1e-6
        # the triangulated points are the scene's up to the scale of t
        tri = r["triangulated"]
        first = j["matches"][:, 0]
        assert tri[first].sum() > 0.9 * len(first) and not np.delete(tri, first).any()
        scale = np.linalg.norm(j["truth"][1])
        assert np.abs(r["P3D"][first][tri[first]].astype(np.float64) * scale - j["X"][tri[first]]).max() < 1e-2


def test_no_parallax_returns_false():
    for key in sc.keys():
        if key[0] == "no_parallax":
            r = sc.result(*key)
            assert not r["ok"] and r["model"] in (1, 2)
            assert not r["triangulated"].any() and not r["P3D"].any() and not r["R21"].any() and not r["t21"].any()


@pytest.mark.parametrize("key", sc.keys() + [sc.MAIN["general"] + (0.0,), sc.MAIN["planar"] + (0.0,)], ids=lambda k: "_".join(map(str, k)))
def test_array_forms_equal_the_sequential_text(key):
    """Initialize's control flow twice: arg-max, second-largest, thresholds on cosines -- and `>` from 0, bestGood / secondBestGood, the
    else-if chain, nsimilar, parallax in degrees through acos"""
    j, tab, r = sc.job(*key), sc.table(*key), sc.result(*key)
    ok, model, R, t, P, tri = im.sequential(j, tab)
    assert ok == r["ok"] and model == r["model"]
    assert P.tobytes() == r["P3D"].tobytes() and tri.tobytes() == r["triangulated"].tobytes()
    if ok:
        assert im.canon(R).tobytes() == r["R21"].tobytes() and im.canon(t).tobytes() == r["t21"].tobytes()


def test_acos_thresholds():
    """for the float just below and at c*, the host expression decides as the comparison does, for `>` and `>=` and several minima"""
    for mp in (1.0, 0.5, 2.0, 0.0, 5.0):
        for ge in (False, True):
            thr = im.cos_threshold(mp, ge)
            below = np.nextafter(thr, f32(-2.0), dtype=f32)
            above = np.nextafter(thr, f32(2.0), dtype=f32)
            for c in (below, thr, above, f32(-1.0), f32(0.0), f32(0.9), f32(1.0)):
                if not -1.0 <= c <= 1.0:
                    continue
                d = im.degrees(c)
                want = bool(d >= f32(mp)) if ge else bool(d > f32(mp))
                assert im.parallax_passes(c, thr) == want, (mp, ge, c)
    assert im.cos_threshold(1.0, True) >= im.cos_threshold(1.0, False)
    assert abs(float(im.cos_threshold(1.0, False)) - np.cos(np.radians(1.0))) < 1e-6
    assert not im.parallax_passes(im.QNAN, im.cos_threshold(1.0, True))


def test_degenerate_row_keeps_the_nan_score_and_the_open_gate():
    """points 4 and 5: a singular H21i inverts to ZEROS, chiSquare1 is NaN, the score is NaN and bIn stays true"""
    j = sc.degenerate_job()
    sh, H21, bh, sf, F21, bf = im.table(j)
    assert sh[:1].view(np.uint32)[0] == 0x7FC00000 and np.isfinite(sh[1])
    assert not H21[0].reshape(3, 3)[:, :2].any() and H21[0][8] == 1.0
    assert not im.inv3(H21[0].reshape(3, 3)).any()
    assert int(bh[0, 0]) & 0xFF == 0xFF                   # chiSquare2 of the eight is 0: only an open first gate lets them in
    assert np.isnan(sf[0]) or sf[0] >= 0
    assert np.count_nonzero(F21[0]) <= 2                  # Fpre has one entry: no completion of the zero singular values
    ch = im.choose((sh, H21, bh, sf, F21, bf))
    assert ch["best_h"] == -1 and ch["SH"] == 0 and ch["best_f"] == 1 and ch["model"] == 2   # a NaN never wins
    assert im.best_of(np.array([np.nan, np.nan], f32)) == (-1, f32(0.0))
    assert im.best_of(np.array([0.0, 2.0, np.nan, 2.0, 1.0], f32))[0] == 1   # the earliest strictly greatest


def test_a_job_without_a_score_reconstructs_nothing():
    """point 6: no hypothesis scores above 0 -> model 0, ok false, an all-false mask"""
    j = sc.scoreless_job()
    tab = im.table(j)
    assert not tab[0].any() and not tab[3].any() and not tab[2].any() and not tab[5].any()
    r = im.initialize(j, tab)
    assert r["model"] == 0 and not r["ok"] and r["best_h"] == -1 and r["best_f"] == -1 and r["winner"] == -1
    assert not r["M"].any() and not r["P3D"].any() and not r["triangulated"].any() and not r["n_good"].any()
    assert im.sequential(j, tab)[:2] == (False, 0)


def test_mask_bits_round_trip():
    rng = np.random.Generator(np.random.PCG64(3))
    for n in (8, 63, 64, 65, 130, 257):
        flags = rng.uniform(size=n) < 0.5
        flags[-1] = True
        w = im.mask_words(flags)
        assert len(w) == (n + 63) // 64 and (im.mask_bools(w, n) == flags).all()
        assert n % 64 == 0 or int(w[-1]) >> (n % 64) == 0
    for key in (sc.MAIN["general"], ("general", 65, 65)):
        n, tab = key[1], sc.table(*key)
        for bits in (tab[2], tab[5]):
            assert n % 64 == 0 or not (bits[:, -1] >> np.uint64(n % 64)).any()
            assert (im.mask_words(im.mask_bools(bits[0], n)) == bits[0]).all()


def _abi_job(pkg, j):
    return pkg.orbx._mono_init_job(j, "test")


def test_refusals(pkg):
    """ORBX_E_INVALID before any device work: no GPU is needed to be refused"""
    j = sc.job("general", 65, 5)
    tab = sc.table("general", 65, 5)

    def refused(word=None, call="hyp", **over):
        jj = dict(j, **over)
        with pytest.raises(pkg.OrbxError) as ei:
            if call == "hyp":
                pkg.mono_init_hypotheses(jj)
            elif call == "init":
                pkg.mono_init_initialize(jj)
            else:
                pkg.mono_init_reconstruct(jj, 2, tab[4][0], np.zeros((len(jj["matches"]) + 63) // 64, np.uint64))
        assert ei.value.code == -1, str(ei.value)
        assert word is None or word in str(ei.value), str(ei.value)

    for call in ("hyp", "init", "rec"):
        refused("n = 7", call, matches=j["matches"][:7], samples=[[0, 1, 2, 3, 4, 5, 6, 6]])              # n outside [8, 8192]
        big = np.stack([np.arange(8193), np.arange(8193)], 1)
        refused("n = 8193", call, matches=big, xy1=np.ones((9000, 2), f32), xy2=np.ones((9000, 2), f32))
        refused("n1", call, xy1=j["xy1"][:64], matches=np.stack([np.arange(65) % 64, j["matches"][:, 1]], 1))   # n1 outside [n, 65535]
        refused("n2", call, xy2=np.ones((65536, 2), f32))
        for bad in ((len(j["xy1"]), 0), (-1, 0)):                                                          # a match index out of range
            ma = j["matches"].copy(); ma[64] = (bad[0], ma[64, 1])
            refused("outside its frame", call, matches=ma)
        ma = j["matches"].copy(); ma[3, 1] = len(j["xy2"])
        refused("outside its frame", call, matches=ma)
        ma = j["matches"].copy(); ma[5, 0] = ma[4, 0]
        refused("strictly rising", call, matches=ma)
    for call in ("hyp", "init"):
        refused("n_hyp", call, samples=np.zeros((0, 8), np.int32))                                        # n_hyp outside [1, 1024]
        refused("n_hyp", call, samples=np.tile(np.arange(8, dtype=np.int32), (1025, 1)))
        for bad in (65, -1):                                                                               # a sample index outside [0, n)
            sa = j["samples"].copy(); sa[4, 7] = bad
            refused("outside", call, samples=sa)
        sa = j["samples"].copy(); sa[2, 6] = sa[2, 1]                                                      # two equal indices in a row
        refused("equal", call, samples=sa)
    with pytest.raises(pkg.OrbxError) as ei:                                                               # model outside {1, 2}
        pkg.mono_init_reconstruct(j, 0, tab[4][0], tab[5][0])
    assert ei.value.code == -1 and "model" in str(ei.value)
    hi = tab[5][0].copy(); hi[-1] |= np.uint64(1) << np.uint64(1)                                          # a mask bit at n = 65
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.mono_init_reconstruct(j, 2, tab[4][0], hi)
    assert ei.value.code == -1 and "mask" in str(ei.value)

    # NULL arguments, on the ABI itself
    L, ox = pkg.lib(), pkg.orbx
    assert L.orbx_mono_init_hypotheses(0, None) == -1
    for name in ("xy1", "xy2", "matches", "samples", "score_h", "score_f", "H21", "F21", "bits_h", "bits_f"):
        J, keep, out = _abi_job(pkg, j)
        setattr(J, name, None)
        assert L.orbx_mono_init_hypotheses(0, C.byref(J)) == -1, name
    J, keep, out = _abi_job(pkg, j)
    P3D, tri = np.zeros((J.n1, 3), f32), np.zeros(J.n1, np.uint8)
    M, mask = np.ascontiguousarray(tab[4][0]), np.ascontiguousarray(tab[5][0])
    good = ox.MonoInitRecon(P3D=P3D.ctypes.data, triangulated=tri.ctypes.data)
    assert L.orbx_mono_init_reconstruct(0, None, 2, M.ctypes.data, mask.ctypes.data, C.byref(good)) == -1
    assert L.orbx_mono_init_reconstruct(0, C.byref(J), 2, None, mask.ctypes.data, C.byref(good)) == -1
    assert L.orbx_mono_init_reconstruct(0, C.byref(J), 2, M.ctypes.data, None, C.byref(good)) == -1
    assert L.orbx_mono_init_reconstruct(0, C.byref(J), 2, M.ctypes.data, mask.ctypes.data, None) == -1
    assert L.orbx_mono_init_reconstruct(0, C.byref(J), 2, M.ctypes.data, mask.ctypes.data, C.byref(ox.MonoInitRecon(P3D=P3D.ctypes.data))) == -1
    res = ox.MonoInitResult(P3D=P3D.ctypes.data, triangulated=tri.ctypes.data)
    assert L.orbx_mono_init_initialize(0, None, C.byref(res)) == -1
    assert L.orbx_mono_init_initialize(0, C.byref(J), None) == -1
    assert L.orbx_mono_init_initialize(0, C.byref(J), C.byref(ox.MonoInitResult(triangulated=tri.ctypes.data))) == -1
    for name in ("xy1", "xy2", "matches", "samples"):
        J, keep, out = _abi_job(pkg, j)
        setattr(J, name, None)
        assert L.orbx_mono_init_initialize(0, C.byref(J), C.byref(res)) == -1, name


def test_the_mirror_draws_the_reference_sets(pkg):
    """mono_init_draw_sets is :93-111 over DUtils::Random: rows of eight distinct indices, reproducible from the seed"""
    a = pkg.mono_init_draw_sets(40, 7, pkg.DUtilsRandom(0))
    b = pkg.mono_init_draw_sets(40, 7, pkg.DUtilsRandom(0))
    assert a.shape == (7, 8) and (a == b).all() and a.min() >= 0 and a.max() < 40
    assert all(len(set(row)) == 8 for row in a.tolist())
    assert sorted(pkg.mono_init_draw_sets(8, 1, pkg.DUtilsRandom(0))[0].tolist()) == list(range(8))
