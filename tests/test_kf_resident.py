"""Resident keyframes for the projection searches whose target is a keyframe (include/orbx.h: orbx_frame_window_best, _window_best_batch,
_search_by_sim3, _search_by_projection_sim3): Fuse x2 (reference src/ORBmatcher.cc:873-1164), SearchBySim3 (:1166-1394) and the Sim3
SearchByProjection (:305-415) with the keyframe given as an orbx_frame handle.  CPU: the ABI surface, its refusals before any device call,
the adaptor driver builds.  GPU: every resident call equals its host-pointer twin and the CPU oracle exactly -- single calls (windows of
more than 64 candidates, point counts that are no multiple of 4), ties (the first candidate in GetFeaturesInArea's order wins), batches
of mixed jobs in one launch, one large job, two threads on one keyframe; the adaptor (KeyFrameFrames, FuseBatch) through its driver."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from test_projection import POP, _scene, _sim3_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ["orbx_frame_window_best", "orbx_frame_window_best_batch", "orbx_frame_search_by_projection_sim3", "orbx_frame_search_by_sim3"]
PARAMS = [(3.0, 1, 50), (4.0, 0, 50), (7.5, 0, 100), (12.0, 1, 50)]          # (th, chi2, max_dist)
SCENES = {41: (300, 257, False), 42: (600, 401, True), 43: (1500, 1203, True)}


@functools.lru_cache(maxsize=None)
def _kf_scene(seed):
    """(keyframe, p2, sf, inv_sigma2): the scene's points with aux = u - 8, as test_hip_other_searches_parity builds them"""
    n_cur, n_pts, dense = SCENES[seed]
    cur, pts, sf = _scene(seed, n_cur, n_pts, dense=dense)
    p2 = dict(pts); p2["aux"] = (pts["u"] - 8).astype(f32)
    return cur, p2, sf, (1.0 / (sf * sf)).astype(f32)


_ORACLE = {}


def _expected(oracle, key, cur, p2, sf, inv_s2, th, chi2, md):
    """the oracle's window_best, computed once per (scene, parameters) and shared by the tests"""
    k = (key, th, chi2, md)
    if k not in _ORACLE:
        bi, bd, n = oracle.window_best(cur, p2, sf, inv_s2, th, chi2, md)
        bi.setflags(write=False); bd.setflags(write=False)
        _ORACLE[k] = (bi, bd, n)
    return _ORACLE[k]


def _frame_only(cur):
    return {k: cur[k] for k in ("x", "y", "octave", "angle", "u_right", "desc", "bounds")}


def _round_half_away(a):
    return (np.sign(a) * np.floor(np.abs(a.astype(np.float64)) + 0.5)).astype(np.int64)


def _windows(cur, pts, sf, th, max_dist):
    """numpy restatement of the window of every point (Frame::GetFeaturesInArea's cell range, the box, levels [l-1, l], no chi2 gate):
    -> (features in the window's cells, admissible candidates at the best distance, the first of them in traversal order), per point"""
    mnx, mny, mxx, mxy = [f32(v) for v in cur["bounds"]]
    inv_w = f32(f32(64) / f32(mxx - mnx)); inv_h = f32(f32(48) / f32(mxy - mny))
    px = _round_half_away((cur["x"] - mnx).astype(f32) * inv_w); py = _round_half_away((cur["y"] - mny).astype(f32) * inv_h)
    ingrid = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    order = np.lexsort((np.arange(len(px)), py, px))                     # traversal: column, row, position in the cell
    n = len(pts["u"])
    in_cells = np.zeros(n, np.int64); at_best = np.zeros(n, np.int64); first = np.full(n, -1, np.int64)
    for i in range(n):
        if not pts["valid"][i]:
            continue
        u, v, lvl = f32(pts["u"][i]), f32(pts["v"][i]), int(pts["level"][i])
        if not (u >= mnx and u < mxx and v >= mny and v < mxy):
            continue
        r = f32(f32(th) * sf[lvl])
        cx0 = max(0, int(np.floor(f32(f32(f32(u - mnx) - r) * inv_w)))); cx1 = min(63, int(np.ceil(f32(f32(f32(u - mnx) + r) * inv_w))))
        cy0 = max(0, int(np.floor(f32(f32(f32(v - mny) - r) * inv_h)))); cy1 = min(47, int(np.ceil(f32(f32(f32(v - mny) + r) * inv_h))))
        if cx0 >= 64 or cx1 < 0 or cy0 >= 48 or cy1 < 0:
            continue
        cells = ingrid & (px >= cx0) & (px <= cx1) & (py >= cy0) & (py <= cy1)
        in_cells[i] = cells.sum()
        ok = cells & (cur["octave"] >= lvl - 1) & (cur["octave"] <= lvl) & (np.abs((cur["x"] - u).astype(f32)) < r) & (np.abs((cur["y"] - v).astype(f32)) < r)
        cand = order[ok[order]]
        if len(cand) == 0:
            continue
        d = POP[cur["desc"][cand] ^ pts["desc"][i]].sum(axis=1)
        if d.min() <= max_dist:
            at_best[i] = (d == d.min()).sum()
            first[i] = cand[np.argmin(d)]                                 # argmin: the first minimum
    return in_cells, at_best, first


# ------------------------------------------------------------------------------------------------ CPU

def test_new_symbols_exported(pkg):
    import __graft_entry__ as ge
    ge.build()
    L = C.CDLL(pkg.lib_path())
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr, n
        assert hasattr(L, n), n
    assert "orbx_window_job" in hdr
    for m in ("FuseResident", "FuseResidentBatch", "SearchByProjectionSim3Resident", "SearchBySim3Resident"):
        assert callable(getattr(pkg.ORBmatcher, m)), m


def test_refusals_need_no_device(pkg):
    """NULL and range refusals come back as ORBX_E_INVALID before any device call (the keyframe handle is never read: a fake one serves)"""
    L = pkg.lib()
    fake = C.c_void_p(4096)
    cur, p2, sf, inv_s2 = _kf_scene(41)
    pts, keep = pkg.ORBmatcher._points(p2)
    n = pts.n
    bi = np.full(n, -1, np.int32); bd = np.full(n, 256, np.int32); nf = C.c_int()
    sfp, sgp = sf.ctypes.data, inv_s2.ctypes.data

    def invalid(rc):
        assert rc == -1, rc
        assert len(L.orbx_last_error()) > 0

    wb = L.orbx_frame_window_best
    invalid(wb(None, C.byref(pts), sfp, sgp, 8, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))       # NULL handle
    invalid(wb(fake, None, sfp, sgp, 8, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))               # NULL points
    invalid(wb(fake, C.byref(pts), None, sgp, 8, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))      # NULL scale factors
    invalid(wb(fake, C.byref(pts), sfp, sgp, 8, 3.0, 1, 50, None, bd.ctypes.data, C.byref(nf)))                 # NULL output
    invalid(wb(fake, C.byref(pts), sfp, None, 8, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))      # chi2 without inv_sigma2
    for md in (-1, 257):
        invalid(wb(fake, C.byref(pts), sfp, sgp, 8, 3.0, 1, md, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))
    for nl in (0, 17):
        invalid(wb(fake, C.byref(pts), sfp, sgp, nl, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))
    lv = int(p2["level"][p2["valid"] == 1].max())
    invalid(wb(fake, C.byref(pts), sfp, sgp, lv, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))      # a valid point at level >= nlevels
    bad = dict(p2); bad["level"] = p2["level"].copy(); bad["valid"] = p2["valid"].copy(); bad["level"][0] = -1; bad["valid"][0] = 1
    pb, kb = pkg.ORBmatcher._points(bad)
    invalid(wb(fake, C.byref(pb), sfp, sgp, 8, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))
    noaux = dict(p2); noaux["aux"] = None
    pa, ka = pkg.ORBmatcher._points(noaux)
    invalid(wb(fake, C.byref(pa), sfp, sgp, 8, 3.0, 1, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))        # chi2 needs aux
    nodesc = dict(p2); nodesc["desc"] = None
    pd, kd = pkg.ORBmatcher._points(nodesc)
    invalid(wb(fake, C.byref(pd), sfp, None, 8, 3.0, 0, 50, bi.ctypes.data, bd.ctypes.data, C.byref(nf)))
    # the batch
    J = pkg.orbx.WindowJob
    jobs = (J * 2)()
    for w in jobs:
        w.kf = fake.value; w.pts = C.pointer(pts); w.scale_factors = sfp; w.inv_sigma2 = sgp; w.nlevels = 8; w.th = 3.0; w.chi2 = 1; w.max_dist = 50
        w.best_idx = bi.ctypes.data; w.best_dist = bd.ctypes.data
    bt = L.orbx_frame_window_best_batch
    invalid(bt(None, 1))
    invalid(bt(jobs, 0))
    invalid(bt(jobs, 1025))
    jobs[1].kf = None
    invalid(bt(jobs, 2))
    jobs[1].kf = fake.value; jobs[1].max_dist = 300
    invalid(bt(jobs, 2))
    jobs[1].max_dist = 50
    huge = pkg.orbx.ProjPoints(); huge.n = (1 << 20) + 1
    jobs[1].pts = C.pointer(huge)
    invalid(bt(jobs, 2))
    half = pkg.orbx.ProjPoints.from_buffer_copy(pts); half.n = 1 << 19                      # each job within the limit, their sum beyond it
    lvl0 = np.zeros(1 << 19, np.int32); val0 = np.zeros(1 << 19, np.uint8)
    half.level = lvl0.ctypes.data; half.valid = val0.ctypes.data
    three = (J * 3)()
    for w in three:
        w.kf = fake.value; w.pts = C.pointer(half); w.scale_factors = sfp; w.nlevels = 8; w.th = 3.0; w.max_dist = 50; w.best_idx = bi.ctypes.data
    invalid(bt(three, 3))
    # the two Sim3 searches
    m = np.full(8, -1, np.int32)
    invalid(L.orbx_frame_search_by_projection_sim3(None, None, C.byref(pts), sfp, 8, 10.0, m.ctypes.data, C.byref(nf)))
    invalid(L.orbx_frame_search_by_projection_sim3(fake, None, None, sfp, 8, 10.0, m.ctypes.data, C.byref(nf)))
    invalid(L.orbx_frame_search_by_projection_sim3(fake, None, C.byref(pts), sfp, 8, 10.0, None, C.byref(nf)))
    invalid(L.orbx_frame_search_by_sim3(None, fake, C.byref(pts), C.byref(pts), sfp, sfp, 8, 7.5, m.ctypes.data, C.byref(nf)))
    invalid(L.orbx_frame_search_by_sim3(fake, None, C.byref(pts), C.byref(pts), sfp, sfp, 8, 7.5, m.ctypes.data, C.byref(nf)))
    invalid(L.orbx_frame_search_by_sim3(fake, fake, None, C.byref(pts), sfp, sfp, 8, 7.5, m.ctypes.data, C.byref(nf)))
    invalid(L.orbx_frame_search_by_sim3(fake, fake, C.byref(pts), C.byref(pts), sfp, sfp, 8, 7.5, None, C.byref(nf)))


ADAPTER = [os.path.join(ROOT, "adapter", f) for f in ("ORBextractor.cc", "Frame_stereo.cc", "ORBmatcher_bow.cc", "ORBmatcher_proj.cc", "ORBmatcher_fuse.cc",
                                                       "Frame_bow.cc", "MapPoint_distinctive.cc", "ORBmatcher_batch.cc")]


def _build_kfframe_driver(tmpdir, overlay):
    """tests/adapter_kfframe_driver.cc against plain tests/cvstub, or with tests/cvstub_replace (a Replace that changes the survivor's
    descriptor) in front of it; the eight adaptor sources the other drivers link"""
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_kfframe_driver" + ("_replace" if overlay else ""))
    inc = ["-I", os.path.join(ROOT, "adapter")] + (["-I", os.path.join(ROOT, "tests", "cvstub_replace")] if overlay else []) + \
          ["-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"] + (["-DKFFRAME_REPLACE_CHANGES_DESCRIPTOR"] if overlay else []) + inc +
                          [os.path.join(ROOT, "tests", "adapter_kfframe_driver.cc")] + ADAPTER +
                          ["-L", os.path.join(ROOT, "orb-slam2_amd"), "-lorbx", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "orb-slam2_amd"), "-o", exe])
    return exe


@pytest.mark.parametrize("overlay", [False, True])
def test_kfframe_driver_compiles(tmp_path, overlay):
    _build_kfframe_driver(str(tmp_path), overlay)


# ------------------------------------------------------------------------------------------------ GPU

FLOORS = {41: 156, 42: 302, 43: 1030}      # found at (7.5, 0, 100), from the oracle on these inputs


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [41, 42, 43])
def test_single_call_parity(pkg, oracle, seed):
    cur, p2, sf, inv_s2 = _kf_scene(seed)
    assert len(p2["u"]) % 4 != 0
    kf = pkg.DeviceFrame(_frame_only(cur))
    mt = pkg.ORBmatcher(0.9, True)
    for th, chi2, md in PARAMS:
        sg = inv_s2 if chi2 else None
        bi, bd, n = mt.FuseResident(kf, p2, sf, sg, th, md)
        hbi, hbd, hn = mt.Fuse(cur, p2, sf, sg, th, md)
        ebi, ebd, en = _expected(oracle, seed, cur, p2, sf, inv_s2, th, chi2, md)
        print(seed, th, chi2, md, "found", n, hn, en)
        assert n == hn == en == int((bi >= 0).sum()), (seed, th, chi2, n, hn, en)
        assert (bi == hbi).all() and (bi == ebi).all(), (seed, th, chi2, np.nonzero(bi != ebi)[0][:5])
        assert (bd == hbd).all() and (bd == ebd).all(), (seed, th, chi2, np.nonzero(bd != ebd)[0][:5])
        if (th, chi2, md) == (7.5, 0, 100):
            assert n >= FLOORS[seed], (seed, n)
    if seed in (42, 43):    # the 64-candidates-at-a-time loop takes several trips
        in_cells, _, _ = _windows(cur, p2, sf, 7.5, 100)
        print(seed, "largest window", in_cells.max())
        assert in_cells.max() >= 65, in_cells.max()


@pytest.mark.gpu
def test_ties_first_in_traversal_order_wins(pkg, oracle):
    cur, pts, sf = _scene(48, 600, 401, dense=True)
    cur["desc"][:] = cur["desc"][np.arange(600) % 4]
    pts["desc"][:] = cur["desc"][np.arange(401) % 4]
    p2 = dict(pts); p2["aux"] = (pts["u"] - 8).astype(f32)
    kf = pkg.DeviceFrame(_frame_only(cur))
    bi, bd, n = pkg.ORBmatcher(0.9, True).FuseResident(kf, p2, sf, None, 7.5, 100)
    ebi, ebd, en = oracle.window_best(cur, p2, sf, None, 7.5, 0, 100)
    _, at_best, first = _windows(cur, p2, sf, 7.5, 100)
    tied = at_best >= 2
    print("found", n, en, "tied points", int(tied.sum()))
    assert tied.sum() >= 100, tied.sum()
    assert (bi[tied] == first[tied]).all(), np.nonzero(tied & (bi != first))[0][:5]
    assert n == en and n >= 355 and (bi == ebi).all() and (bd == ebd).all()
    assert (first == ebi).all()                                          # the numpy restatement agrees with the oracle everywhere


def _slice(d, n):
    return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in d.items()}


@pytest.mark.gpu
def test_batch_of_mixed_jobs(pkg, oracle):
    c41, p41, sf, inv_s2 = _kf_scene(41)
    c43, p43, _, _ = _kf_scene(43)
    c1 = _slice(c43, 1)
    near = _slice(p43, 3)
    near["u"] = np.full(3, c1["x"][0], f32) + np.array([0.5, -1.0, 40.0], f32); near["v"] = np.full(3, c1["y"][0], f32)
    near["aux"] = (near["u"] - 8).astype(f32); near["level"] = np.full(3, c1["octave"][0], np.int32); near["valid"] = np.ones(3, np.uint8)
    near["desc"] = np.repeat(c1["desc"], 3, axis=0)
    c0 = _slice(c43, 0)
    f300, f1500, f1, f0 = [pkg.DeviceFrame(_frame_only(c)) for c in (c41, c43, c1, c0)]
    assert (f300.n, f1500.n, f1.n, f0.n) == (300, 1500, 1, 0)
    spec = [(f300, c41, p41, 7.5, 0, 100), (f1500, c43, p43, 3.0, 1, 50), (f1500, c43, _slice(p43, 5), 4.0, 0, 50), (f1, c1, near, 12.0, 1, 50),
            (f300, c41, _slice(p41, 0), 3.0, 1, 50), (f0, c0, _slice(p41, 1), 7.5, 0, 100), (f300, c41, _slice(p41, 1), 12.0, 1, 64)]
    assert sorted(len(s_[2]["u"]) for s_ in spec) == [0, 1, 1, 3, 5, 257, 1203]
    mt = pkg.ORBmatcher(0.9, True)
    jobs = [dict(kf=kf, points=p, scaleFactors=sf, invLevelSigma2=inv_s2 if chi2 else None, th=th, max_dist=md) for kf, _, p, th, chi2, md in spec]
    res = mt.FuseResidentBatch(jobs)
    total = 0
    for (kf, c, p, th, chi2, md), (bi, bd, n) in zip(spec, res):
        np_ = len(p["u"])
        assert len(bi) == np_ and n == int((bi >= 0).sum())
        if np_ == 0 or kf.n == 0:
            assert n == 0 and (bi == -1).all() and (bd == 256).all()
            continue
        sbi, sbd, sn = mt.FuseResident(kf, p, sf, inv_s2 if chi2 else None, th, md)
        ebi, ebd, en = oracle.window_best(c, p, sf, inv_s2, th, chi2, md)
        assert n == sn == en, (np_, th, n, sn, en)
        assert (bi == sbi).all() and (bi == ebi).all() and (bd == sbd).all() and (bd == ebd).all(), (np_, th)
        total += n
    assert res[3][2] == 2 and list(res[3][0]) == [0, 0, -1]              # the one-feature keyframe: two points see it, the third is 40 px away
    assert res[0][2] >= FLOORS[41] and total >= 400                      # (435 by the oracle)
    # a batch of nothing but empty jobs: no launch, all -1
    e = mt.FuseResidentBatch([jobs[4], jobs[5]])
    assert all(n == 0 and (bi == -1).all() for bi, _, n in e)


@pytest.mark.gpu
def test_large_single_job(pkg, oracle):
    """Fuse(mpCurrentKeyFrame, vpFuseCandidates), src/LocalMapping.cc:579: tens of thousands of points into one keyframe"""
    cur, pts, sf = _scene(44, 1500, 20011, dense=True)
    p2 = dict(pts); p2["aux"] = (pts["u"] - 8).astype(f32)
    inv_s2 = (1.0 / (sf * sf)).astype(f32)
    kf = pkg.DeviceFrame(_frame_only(cur))
    bi, bd, n = pkg.ORBmatcher(0.9, True).FuseResident(kf, p2, sf, inv_s2, 3.0, 50)
    ebi, ebd, en = oracle.window_best(cur, p2, sf, inv_s2, 3.0, 1, 50)
    print("found", n, en)
    assert n == en and n >= 4000 and (bi == ebi).all() and (bd == ebd).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,floor", [(41, 113), (42, 185), (43, 576)])
def test_search_by_projection_sim3_resident(pkg, oracle, seed, floor):
    cur, p2, sf, _ = _kf_scene(seed)
    kf = pkg.DeviceFrame(_frame_only(cur))
    mt = pkg.ORBmatcher(0.9, True)
    got, n = mt.SearchByProjectionSim3Resident(kf, cur["occupied"], p2, sf, 10.0)
    exp, en = oracle.search_by_projection_sim3(cur, p2, sf, 10.0)
    hg, hn = mt.SearchByProjectionSim3(cur, p2, sf, 10.0)
    print(seed, "matches", n, en)
    assert n == en == hn and n >= floor and (got == exp).all() and (got == hg).all()
    occ2 = (np.arange(kf.n) % 3 == 0).astype(np.uint8)                   # the same frame, another vpMatched
    got2, n2 = mt.SearchByProjectionSim3Resident(kf, occ2, p2, sf, 10.0)
    exp2, en2 = oracle.search_by_projection_sim3(dict(cur, occupied=occ2), p2, sf, 10.0)
    assert n2 == en2 and (got2 == exp2).all() and not (got2 == got).all()
    got3, n3 = mt.SearchByProjectionSim3Resident(kf, None, p2, sf, 10.0)
    exp3, en3 = oracle.search_by_projection_sim3(dict(cur, occupied=np.zeros(kf.n, np.uint8)), p2, sf, 10.0)
    assert n3 == en3 and (got3 == exp3).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,floor", [(46, 300, 209), (47, 700, 482)])
def test_search_by_sim3_resident(pkg, oracle, seed, n, floor):
    c1, c2, p12, p21, sf = _sim3_scene(seed, n)
    k1, k2 = pkg.DeviceFrame(_frame_only(c1)), pkg.DeviceFrame(_frame_only(c2))
    mt = pkg.ORBmatcher(0.75, True)
    got, gn = mt.SearchBySim3Resident(k1, k2, p12, p21, sf, sf, 7.5)
    exp, en = oracle.search_by_sim3(c1, c2, p12, p21, sf, sf, 7.5)
    hg, hn = mt.SearchBySim3(c1, c2, p12, p21, sf, sf, 7.5)
    print(seed, "found", gn, en)
    assert gn == en == hn and gn >= floor and (got == exp).all() and (got == hg).all()
    with pytest.raises(pkg.OrbxError) as ei:
        bad = {k: v[:-1] if isinstance(v, np.ndarray) else v for k, v in p12.items()}
        mt.SearchBySim3Resident(k1, k2, bad, p21, sf, sf, 7.5)
    assert ei.value.code == -1


@pytest.mark.gpu
def test_two_threads_one_keyframe(pkg, oracle):
    """LocalMapping and LoopClosing search one keyframe at the same time: the calls only read the handle"""
    cur, p2, sf, inv_s2 = _kf_scene(42)
    kf = pkg.DeviceFrame(_frame_only(cur))
    exp = {c: _expected(oracle, 42, cur, p2, sf, inv_s2, th, c, md) for th, c, md in (PARAMS[0], PARAMS[2])}
    bad = []

    def work(th, chi2, md):
        mt = pkg.ORBmatcher(0.9, True)
        try:
            for _ in range(50):
                bi, bd, n = mt.FuseResident(kf, p2, sf, inv_s2 if chi2 else None, th, md)
                ebi, ebd, en = exp[chi2]
                if n != en or not (bi == ebi).all() or not (bd == ebd).all():
                    bad.append((th, n, en))
        except Exception as e:      # noqa: BLE001
            bad.append(repr(e))
        finally:
            pkg.orbx.thread_release()

    ts = [threading.Thread(target=work, args=PARAMS[0]), threading.Thread(target=work, args=PARAMS[2])]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad, bad[:3]


def _run_driver(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = run.stdout + run.stderr
    print(out)
    assert run.returncode == 0, out
    return dict(line.split(" ", 1) for line in run.stdout.strip().splitlines() if " " in line), out


@pytest.mark.gpu
def test_adaptor_resident_keyframes(tmp_path):
    """registered keyframes == the unregistered path for the four searches; a recycled address is rebuilt; FuseBatch == the loop"""
    v, out = _run_driver(_build_kfframe_driver(str(tmp_path), False))
    assert v["registered_equal"] == "1" and v["recycled_rebuilt"] == "1" and v["recycled_equal"] == "1", out
    assert v["batch_equal"] == "1" and v["batch_launches"] == "1" and v["batch_researched"] == "0", out
    assert int(v["batch_targets"]) == 5 and int(v["batch_points"]) >= 300, out
    assert int(v["loop_replace_new_by_old"]) >= 1 and int(v["loop_replace_old_by_new"]) >= 1 and int(v["loop_add_observation"]) >= 1, out


@pytest.mark.gpu
def test_adaptor_fuse_batch_with_descriptor_changing_replace(tmp_path):
    """a Replace during target t's surgery changes the survivor's descriptor: the points that differ are searched again against target t+1"""
    v, out = _run_driver(_build_kfframe_driver(str(tmp_path), True))
    assert v["batch_equal"] == "1" and v["batch_launches"] == "1" and int(v["batch_researched"]) >= 1, out
    assert int(v["loop_replace_new_by_old"]) >= 1 and int(v["loop_replace_old_by_new"]) >= 1 and int(v["loop_add_observation"]) >= 1, out
