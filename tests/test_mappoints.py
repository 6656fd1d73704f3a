"""Resident map points (include/orbx.h: orbx_mappoints): the table (set / read / capacity / refusals) and Frame::isInFrustum on the
device, compared with tests/frustum_model.py field by field -- floats as bit patterns -- on random local maps and on points placed on
every edge of every rejection rule.  CPU: the ABI surface and its refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import frustum_model as fm
import localmap_scene as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ["orbx_mappoints_create", "orbx_mappoints_destroy", "orbx_mappoints_capacity", "orbx_mappoints_set", "orbx_mappoints_read",
               "orbx_mappoints_frustum", "orbx_frame_search_local_points"]
FIELDS = ("in_view", "u", "v", "xr", "level", "view_cos")


def _same(got, exp, tag):
    for k in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, k, np.nonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))[0][:5])


# ------------------------------------------------------------------------------------------------ CPU

def test_new_symbols_exported_and_typed(pkg):
    import __graft_entry__ as ge
    ge.build()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr, n
        assert getattr(L, n).argtypes is not None, n
    assert hasattr(pkg, "MapPoints") and callable(pkg.DeviceFrame.search_local_points)
    for m in ("set", "read", "frustum"):
        assert callable(getattr(pkg.MapPoints, m)), m


def test_malformed_arguments_rejected(pkg):
    L = pkg.lib()
    h = C.c_void_p()
    assert L.orbx_mappoints_create(0, 0, C.byref(h)) == -1 and len(L.orbx_last_error()) > 0
    assert L.orbx_mappoints_create(0, 16, None) == -1
    assert L.orbx_mappoints_capacity(None) == -1
    L.orbx_mappoints_destroy(None)
    s = (C.c_int32 * 2)(0, 1); g = (C.c_float * 16)(); iv = (C.c_uint8 * 2)(); m = (C.c_int32 * 8)(); n = C.c_int()
    assert L.orbx_mappoints_set(None, s, 2, g, None, None) == -1
    assert L.orbx_mappoints_read(None, s, 2, g, None) == -1
    assert L.orbx_mappoints_frustum(None, s, iv, 2, g, g, 0.5, 0.18, 8, iv, None, None, None, None, None) == -1
    assert L.orbx_frame_search_local_points(None, None, None, s, iv, 2, g, g, 0.5, 0.18, g, 8, 1.0, 0.8, m, C.byref(n), iv) == -1
    if L.orbx_device_count() == 0:
        with pytest.raises(pkg.OrbxError) as ei:
            pkg.MapPoints(16)
        assert ei.value.code == -4                                               # no device: no host table stands in


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def table(pkg):
    """512 slots; a 300-point local map in slots with gaps, in no particular order"""
    frame, geom, desc, has_obs, po = ls.scene(11)
    rng = np.random.Generator(np.random.PCG64(1))
    slots = rng.permutation(500)[:len(geom)].astype(np.int32)
    mp = pkg.MapPoints(512)
    assert mp.capacity == 512
    mp.set(slots, geom, desc)
    elig = (rng.random(len(geom)) < 0.9).astype(np.uint8)
    exp = fm.frustum(geom, elig, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    return dict(mp=mp, slots=slots, geom=geom, desc=desc, pose=po, elig=elig, exp=exp)


@pytest.mark.gpu
def test_frustum_equals_the_model(table):
    t = table
    got = t["mp"].frustum(t["slots"], t["elig"], t["pose"], ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    _same(got, t["exp"], "random")
    iv = t["exp"]["in_view"]
    assert 150 < iv.sum() < 290 and len(set(t["exp"]["level"][iv == 1].tolist())) >= 6   # the scene exercises the rules and the levels
    g, d = t["mp"].read(t["slots"])
    assert g.tobytes() == t["geom"].tobytes() and d.tobytes() == t["desc"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_workgroup_edges(table, n):
    t = table
    got = t["mp"].frustum(t["slots"][:n], t["elig"][:n], t["pose"], ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    _same(got, {k: t["exp"][k][:n] for k in FIELDS}, n)


@pytest.mark.gpu
def test_descending_slots_and_second_scale_factor(table):
    t = table
    order = np.argsort(-t["slots"])
    got = t["mp"].frustum(t["slots"][order], t["elig"][order], t["pose"], ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    _same(got, {k: t["exp"][k][order] for k in FIELDS}, "descending")
    for factor, nlevels, limit in ((1.1, 12, 0.5), (2.0, 3, 0.8)):
        lsf = f32(np.log(f32(factor)))
        got = t["mp"].frustum(t["slots"], t["elig"], t["pose"], ls.CAM, limit, lsf, nlevels)
        exp = fm.frustum(t["geom"], t["elig"], t["pose"], ls.CAM, limit, lsf, nlevels)
        _same(got, exp, factor)
        assert exp["level"].max() == nlevels - 1


def _edge_points():
    """points on each edge of each rule for IDENTITY / EDGE_CAM (u = 512 * X / Z, dist = Z on the axis): -> geom[n][8], names"""
    up = lambda x: np.nextafter(f32(x), f32(np.inf))
    dn = lambda x: np.nextafter(f32(x), f32(-np.inf))
    thr = fm.level_thresholds(ls.LSF, ls.NLEVELS)
    P = []
    add = lambda name, X, Y, Z, dmin, n, dmax: P.append((name, [X, Y, Z, dmin, n[0], n[1], n[2], dmax]))
    z1 = (0, 0, 1)
    add("z slightly negative", 0, 0, -1e-30, 1e-31, z1, 1e-29)
    add("z -0", 0, 0, -0.0, 0, z1, 1); add("z +0", 0, 0, 0.0, 0, z1, 1)
    add("u on min", 0, 0.5, 1, 0.1, z1, 2); add("u below min", -1e-45, 0.5, 1, 0.1, z1, 2)
    add("u on max", 1.25, 0, 1, 0.1, z1, 2); add("u above max", up(1.25), 0, 1, 0.1, z1, 2)
    add("v on min", 0.5, 0, 1, 0.1, z1, 2); add("v below min", 0.5, -1e-45, 1, 0.1, z1, 2)
    add("v on max", 0, 0.9375, 1, 0.1, z1, 2); add("v above max", 0, up(0.9375), 1, 0.1, z1, 2)
    lo = f32(f32(0.8) * f32(2.5)); hi = f32(f32(1.2) * f32(3.0))
    add("dist on 0.8 dmin", 0, 0, lo, 2.5, z1, 4); add("dist below 0.8 dmin", 0, 0, dn(lo), 2.5, z1, 4)
    add("dist on 1.2 dmax", 0, 0, hi, 1, z1, 3.0); add("dist above 1.2 dmax", 0, 0, up(hi), 1, z1, 3.0)
    add("cos on the limit", 0, 0, 3, 1, (0, 0.8, 0.5), 4); add("cos below the limit", 0, 0, 3, 1, (0, 0.8, dn(0.5)), 4)
    add("cos NaN", 0, 0, 3, 1, (np.nan, 0, 1), 4)
    for k, r in enumerate(thr):
        add(f"ratio on r_{k}", 0, 0, 1, 0.1, z1, r); add(f"ratio under r_{k}", 0, 0, 1, 0.1, z1, dn(r))
    add("level clamps to 0", 0, 0, 1, 0.01, z1, 0.84); add("level clamps to the top", 0, 0, 1, 0.1, z1, 100)
    return np.array([g for _, g in P], f32), [n for n, _ in P], thr


@pytest.mark.gpu
def test_every_edge_of_every_rule(pkg):
    geom, names, thr = _edge_points()
    n = len(geom)
    mp = pkg.MapPoints(512)
    slots = (np.arange(n, dtype=np.int32) * 3 + 7) % 512
    mp.set(slots, geom, np.zeros((n, 32), np.uint8))
    ones = np.ones(n, np.uint8)
    got = mp.frustum(slots, ones, ls.IDENTITY, ls.EDGE_CAM, 0.5, ls.LSF, ls.NLEVELS)
    exp = fm.frustum(geom, ones, ls.IDENTITY, ls.EDGE_CAM, 0.5, ls.LSF, ls.NLEVELS)
    _same(got, exp, "edges")
    # the model places every case on the side its name says, so the comparison above is about those sides
    at = {nm: i for i, nm in enumerate(names)}
    for nm in names:
        inside = not any(w in nm for w in ("below", "above", "z ", "NaN"))
        assert exp["in_view"][at[nm]] == inside, nm
    assert exp["u"][at["u on max"]] == f32(640) and exp["u"][at["u on min"]] == f32(0)
    assert exp["v"][at["v on max"]] == f32(480) and exp["v"][at["v on min"]] == f32(0)
    assert exp["view_cos"][at["cos on the limit"]] == f32(0.5)
    for k in range(len(thr)):
        assert exp["level"][at[f"ratio on r_{k}"]] == k + 1 and exp["level"][at[f"ratio under r_{k}"]] == k
    assert exp["level"][at["level clamps to 0"]] == 0 and exp["level"][at["level clamps to the top"]] == ls.NLEVELS - 1


@pytest.mark.gpu
def test_set_halves_refusals_and_capacity(pkg):
    frame, geom, desc, has_obs, po = ls.scene(12, n_pts=40)
    mp = pkg.MapPoints(64)
    slots = np.arange(40, dtype=np.int32)[::-1].copy()
    ones = np.ones(40, np.uint8)
    for g1, d1 in ((geom[:1], None), (None, desc[:1])):                           # a half left out that the slot never had
        with pytest.raises(pkg.OrbxError) as ei:
            mp.set(slots[:1], g1, d1)
        assert ei.value.code == -1
    mp.set(slots, geom, desc)
    exp = fm.frustum(geom, ones, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    _same(mp.frustum(slots, ones, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS), exp, "before")
    # a slot that is not set: accepted when not eligible, refused when eligible; so is a slot out of range
    s2 = slots.copy(); s2[3] = 50
    e2 = ones.copy(); e2[3] = 0
    got = mp.frustum(s2, e2, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    x2 = fm.frustum(geom, e2, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    _same(got, x2, "not eligible, not set")
    s2[3] = 1 << 30
    _same(mp.frustum(s2, e2, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS), x2, "not eligible, out of range")
    for bad in (50, 64, -1):
        s2[3] = bad
        with pytest.raises(pkg.OrbxError) as ei:
            mp.frustum(s2, ones, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
        assert ei.value.code == -1, bad
    # geometry only: bundle adjustment moves point 5 behind the camera and point 6 a little; descriptors stay
    i5 = int(np.nonzero(exp["in_view"])[0][0]); i6 = int(np.nonzero(exp["in_view"])[0][1])
    g2 = geom.copy()
    Ow = po[12:15]
    g2[i5, :3] = Ow - (geom[i5, :3] - Ow)
    g2[i6, :3] = geom[i6, :3] + f32(0.01)
    mp.set(slots[[i5, i6]], g2[[i5, i6]], None)
    exp2 = fm.frustum(g2, ones, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    assert exp2["in_view"][i5] == 0 and exp2["in_view"][i6] == 1 and exp2["u"][i6] != exp["u"][i6]
    _same(mp.frustum(slots, ones, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS), exp2, "after the move")
    # descriptor only
    d2 = desc.copy(); d2[7] ^= 0xFF
    mp.set(slots[7:8], None, d2[7:8])
    g, d = mp.read(slots)
    assert g.tobytes() == g2.tobytes() and d.tobytes() == d2.tobytes()
    _same(mp.frustum(slots, ones, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS), exp2, "after the descriptor")
    # the limit: ORBX_E_CAPACITY, and the table is as it was
    for over in ([10, 64], [1 << 20]):
        sl = np.array(over, np.int32)
        with pytest.raises(pkg.OrbxError) as ei:
            mp.set(sl, g2[:len(sl)], d2[:len(sl)])
        assert ei.value.code == -2, over
    with pytest.raises(pkg.OrbxError) as ei:
        mp.set(np.array([4, 4], np.int32), g2[:2], d2[:2])                        # a slot named twice
    assert ei.value.code == -1
    g, d = mp.read(slots)
    assert g.tobytes() == g2.tobytes() and d.tobytes() == d2.tobytes()
    mp.set(np.array([63], np.int32), g2[:1], d2[:1])                             # the last slot is a slot
    g, d = mp.read(np.array([63], np.int32))
    assert g.tobytes() == g2[:1].tobytes() and d.tobytes() == d2[:1].tobytes()


@pytest.mark.gpu
def test_set_larger_than_one_upload(pkg):
    """a set of more records than the staging of one upload holds (65536) goes in two; geometry only, then descriptors only, then both"""
    n = 65536 + 4464
    rng = np.random.Generator(np.random.PCG64(3))
    geom = rng.normal(0, 5, (n, 8)).astype(f32); desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    slots = np.arange(n, dtype=np.int32)[::-1].copy()
    mp = pkg.MapPoints(n)
    mp.set(slots, geom, desc)
    pick = np.concatenate([np.arange(0, 40), np.arange(65530, 65545), np.arange(n - 20, n)])   # both uploads and their seam
    g, d = mp.read(slots[pick])
    assert g.tobytes() == geom[pick].tobytes() and d.tobytes() == desc[pick].tobytes()
    g, d = mp.read(np.sort(slots[pick]))                                         # ascending runs
    back = np.argsort(slots[pick])
    assert g.tobytes() == geom[pick][back].tobytes() and d.tobytes() == desc[pick][back].tobytes()
    mp.set(slots, geom + f32(1), None)
    mp.set(slots, None, ~desc)
    g, d = mp.read(slots[pick])
    assert g.tobytes() == (geom + f32(1))[pick].tobytes() and d.tobytes() == (~desc)[pick].tobytes()
