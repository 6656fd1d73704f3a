"""orbx_mono_init_hypotheses / _reconstruct / _initialize (k_mono_hyp, k_mono_reconstruct, k_mono_decide) against tests/init_model.py,
BIT FOR BIT and without a tolerance: both scores' bit patterns, both matrices, every mask word, the counts, the ranked cosines, the
motions and the points.  Each lane's arithmetic is fixed by the contract of include/orbx.h, the counts are exact integer sums and the
ranked cosine is exact whatever the selection method.  The jobs (tests/init_scene.py) hold n in {8, 63, 64, 65, 130, 257} and n_hyp in
{1, 5, 64, 65, 200} on four scenes."""
import ctypes as C

import numpy as np
import pytest

import init_model as im
import init_scene as sc

GUARD = 0xA5
TABLE = ("score_h", "H21", "bits_h", "score_f", "F21", "bits_f")
RECON = ("ok", "winner", "n_good", "cos_parallax", "R", "t", "P3D", "triangulated")
RESULT = ("ok", "model", "best_h", "best_f", "SH", "SF", "M", "R21", "t21", "parallax", "winner", "n_good", "cos_parallax", "P3D", "triangulated")


def _ids(k):
    return "_".join(map(str, k))


def _table_diff(got, exp, n):
    for name, g, e in zip(TABLE, got, exp):
        if g.tobytes() != e.tobytes():
            gi, ei = g.reshape(len(g), -1), e.reshape(len(e), -1)
            k = int(np.nonzero((gi.view(np.uint8) != ei.view(np.uint8)).any(1))[0][0])
            return f"hypothesis {k}: {name} {gi[k]} != {ei[k]}"
    for bits in (got[2], got[5]):
        if n % 64 and (bits[:, -1] >> np.uint64(n % 64)).any():
            return "mask bits >= n are set"
    return None


def _dict_diff(got, exp, names):
    for name in names:
        g, e = np.asarray(got[name]), np.asarray(exp[name])
        if g.dtype != e.dtype or g.shape != e.shape or g.tobytes() != e.tobytes():
            return f"{name}: {g} != {e}"
    return None


def _guarded_table(pkg, job):
    """orbx_mono_init_hypotheses with every output array inside a larger block of guard bytes, asserting the guards"""
    ox, L = pkg.orbx, pkg.lib()
    J, keep, out = ox._mono_init_job(job, "test")
    blocks = []
    for name, a in zip(TABLE, out):
        blk = np.full(a.nbytes + 128, GUARD, np.uint8)
        setattr(J, name, blk.ctypes.data + 64)
        blocks.append((blk, a))
    assert L.orbx_mono_init_hypotheses(0, C.byref(J)) == 0, L.orbx_last_error()
    res = []
    for blk, a in blocks:
        assert (blk[:64] == GUARD).all() and (blk[64 + a.nbytes:] == GUARD).all(), "written outside the job's arrays"
        res.append(blk[64:64 + a.nbytes].view(a.dtype).reshape(a.shape).copy())
    return tuple(res)


def _guarded_points(pkg, job, call, *args):
    """_reconstruct / _initialize with P3D and triangulated inside guard bytes -> (P3D, triangulated) as the mirror returns them"""
    ox, L = pkg.orbx, pkg.lib()
    J, keep, _ = ox._mono_init_job(job, "test", table=False)
    b3, bt = np.full(12 * J.n1 + 128, GUARD, np.uint8), np.full(J.n1 + 128, GUARD, np.uint8)
    if call == "reconstruct":
        model, M, mask = args
        M, mask = np.ascontiguousarray(M, np.float32), np.ascontiguousarray(mask, np.uint64)
        R = ox.MonoInitRecon(P3D=b3.ctypes.data + 64, triangulated=bt.ctypes.data + 64)
        rc = L.orbx_mono_init_reconstruct(0, C.byref(J), model, M.ctypes.data, mask.ctypes.data, C.byref(R))
    else:
        R = ox.MonoInitResult(P3D=b3.ctypes.data + 64, triangulated=bt.ctypes.data + 64)
        rc = L.orbx_mono_init_initialize(0, C.byref(J), C.byref(R))
    assert rc == 0, L.orbx_last_error()
    for blk in (b3, bt):
        assert (blk[:64] == GUARD).all() and (blk[-64:] == GUARD).all(), "written outside the job's arrays"
    return b3[64:-64].view(np.float32).reshape(J.n1, 3).copy(), bt[64:-64].astype(bool)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sc.keys(), ids=_ids)
def test_table_matches_the_model(pkg, key):
    j, exp = sc.job(*key), sc.table(*key)
    got = pkg.mono_init_hypotheses(j)
    assert _table_diff(got, exp, key[1]) is None, _table_diff(got, exp, key[1])
    again = pkg.mono_init_hypotheses(j)                     # the staging is reused: a second call gives the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    guarded = _guarded_table(pkg, j)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, guarded))


def _masks(tab, col, best, n):
    """the winner's mask (more than 51 accepted on the main scenes), its first 30 set bits (fewer than 51) and the empty mask"""
    full = tab[col][best]
    flags = im.mask_bools(full, n)
    few = np.zeros(n, bool)
    few[np.nonzero(flags)[0][:30]] = True
    return (("full", full), ("few", im.mask_words(few)), ("none", np.zeros_like(full)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["general", "planar", "outliers", "no_parallax"])
def test_reconstruct_matches_the_model(pkg, kind):
    key = sc.MAIN[kind]
    j, tab, r = sc.job(*key), sc.table(*key), sc.result(*key)
    n = key[1]
    seen = set()
    for model, mcol, bcol, best in ((1, 1, 2, r["best_h"]), (2, 4, 5, r["best_f"])):
        for name, mask in _masks(tab, bcol, best, n):
            exp = im.reconstruct(j, model, tab[mcol][best], mask)
            got = pkg.mono_init_reconstruct(j, model, tab[mcol][best], mask)
            assert _dict_diff(got, exp, RECON) is None, (model, name, _dict_diff(got, exp, RECON))
            P, tri = _guarded_points(pkg, j, "reconstruct", model, tab[mcol][best], mask)
            assert P.tobytes() == got["P3D"].tobytes() and (tri == got["triangulated"]).all()
            if name == "none":
                assert not got["ok"] and not got["n_good"].any() and (got["cos_parallax"][:4 if model == 2 else 8] == 1.0).all()
            seen.add((name, "over" if exp["n_good"].max() > 51 else "under"))
    if kind in ("general", "planar"):
        assert ("full", "over") in seen and ("few", "under") in seen     # both sides of min(50, size - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sc.keys() + [sc.MAIN["general"] + (0.0,), sc.MAIN["planar"] + (0.0,)], ids=_ids)
def test_initialize_is_table_then_reconstruct_and_the_model(pkg, key):
    j, exp = sc.job(*key), sc.result(*key)
    got = pkg.mono_init_initialize(j)
    assert _dict_diff(got, exp, RESULT) is None, _dict_diff(got, exp, RESULT)
    tab = pkg.mono_init_hypotheses(j)
    ch = im.choose(tab)
    assert (ch["model"], ch["best_h"], ch["best_f"]) == (got["model"], got["best_h"], got["best_f"])
    assert ch["model"] != 0
    best, M, mask = (ch["best_h"], tab[1], tab[2]) if ch["model"] == 1 else (ch["best_f"], tab[4], tab[5])
    assert got["M"].tobytes() == M[best].tobytes()
    rec = pkg.mono_init_reconstruct(j, ch["model"], M[best], mask[best])
    assert _dict_diff(got, rec, ("ok", "winner", "n_good", "cos_parallax", "P3D", "triangulated")) is None
    if got["ok"]:
        assert got["R21"].tobytes() == rec["R"][rec["winner"]].tobytes() and got["t21"].tobytes() == rec["t"][rec["winner"]].tobytes()
    else:
        assert not got["R21"].any() and not got["t21"].any() and not got["P3D"].any() and not got["triangulated"].any()
    if key[0] == "no_parallax":
        assert not got["ok"] and got["model"] in (1, 2)
    P, tri = _guarded_points(pkg, j, "initialize")
    assert P.tobytes() == got["P3D"].tobytes() and (tri == got["triangulated"]).all()
    again = pkg.mono_init_initialize(j)
    assert _dict_diff(got, again, RESULT) is None


@pytest.mark.gpu
def test_initializer_class_draws_and_initialises(pkg):
    """the mirror's Initializer on the general scene: vMatches12 in, the reference's own draw of mvSets, the tuple of Initialize out"""
    j = sc.job(*sc.MAIN["general"])
    m12 = np.full(len(j["xy1"]), -1, np.int32)
    m12[j["matches"][:, 0]] = j["matches"][:, 1]
    ini = pkg.Initializer(j["xy1"], np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32), 1.0, 200)
    ok, R21, t21, P3D, tri = ini.Initialize(j["xy2"], m12)
    sets = pkg.mono_init_draw_sets(len(j["matches"]), 200, pkg.DUtilsRandom(0))
    assert (ini.sets == sets).all()
    exp = im.initialize(dict(j, samples=sets))
    assert ok == exp["ok"] and exp["model"] == 2
    assert R21.tobytes() == exp["R21"].tobytes() and t21.tobytes() == exp["t21"].tobytes()
    assert P3D.tobytes() == exp["P3D"].tobytes() and (tri == exp["triangulated"]).all()
    ok2, R2, t2, P2, tri2 = ini.Initialize(j["xy2"], m12, samples=j["samples"])
    assert R2.tobytes() == sc.result(*sc.MAIN["general"])["R21"].tobytes()


@pytest.mark.gpu
def test_degenerate_rows_give_the_models_bytes(pkg):
    """points 4, 5 and 6 on the device: the zero inverse, the NaN score with the open gate, the job without a score"""
    j = sc.degenerate_job()
    exp = im.table(j)
    got = pkg.mono_init_hypotheses(j)
    assert _table_diff(got, exp, 40) is None, _table_diff(got, exp, 40)
    assert got[0][:1].view(np.uint32)[0] == 0x7FC00000 and int(got[2][0, 0]) & 0xFF == 0xFF
    assert _dict_diff(pkg.mono_init_initialize(j), im.initialize(j, exp), RESULT) is None
    j = sc.scoreless_job()
    exp = im.table(j)
    got = pkg.mono_init_hypotheses(j)
    assert _table_diff(got, exp, 65) is None and not got[0].any() and not got[3].any()
    r = pkg.mono_init_initialize(j)
    assert _dict_diff(r, im.initialize(j, exp), RESULT) is None
    assert r["model"] == 0 and not r["ok"] and r["winner"] == -1 and not r["P3D"].any()
