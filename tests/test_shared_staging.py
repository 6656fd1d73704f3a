"""The calls that share one per-thread staging context (CallCtx, orb-slam2_amd/csrc/orbx_resident.h), one after another in one thread:
a host-pointer projection search, orbx_frame_create and a resident search, orbx_frame_window_best, orbx_mappoints_set / _frustum,
orbx_frame_search_local_points, orbx_pose_optimize / orbx_frame_pose_optimize, orbx_triangulate_pairs / orbx_frame_triangulate and
orbx_sim3_hypotheses.  They are one context family (one stream, one set of buffers per thread), and what a call returns does not depend
on what the context's buffers held or how large they were when it began.

Every call is made at two sizes.  Small: 64 features / 48 points for the searches, 64 features / 32 slots for the local map, 9
correspondences, one pair between two keyframes of 300 features, 5 hypotheses over 20 points.  Large: 600 / 500, 300 / 600, 257
correspondences, 1414 pairs over 20 neighbours, 64 hypotheses over 300 points.  The requests in bytes, from the formulas of the host code
(a16 = rounded up to 16; a job header of a few hundred bytes is left out where an array dominates):

  blob      small, the largest: orbx_triangulate_pairs, 2 keyframes x 5 arrays x a16(4 x 300) + head = about 13 K (the host-pointer
            search: 3 328 of frame arrays + 2 848 of points = 6 176).  A buffer holds at most twice the largest request: 26 K.
            large: orbx_triangulate_pairs, 21 keyframes x 5 arrays x 1 200 + 8 x 1 414 + head = about 141 K; before it in the large
            round only orbx_sim3_hypotheses (2 x 3 600 + 2 x 1 200 + 768 = about 10 K) and orbx_frame_triangulate (head + 8 x 1 414 =
            about 15 K) have run.  (The keyframes of orbx_frame_triangulate are made beforehand, by another thread.)
  work      small, the largest: orbx_frame_search_local_points, 12 304 + 8 nc + 24 np + 32 + (2 a16(np) + 52 np) = 15 344 (nc = 64, np = 32).
            large: the same call with nc = 300, np = 600: 61 552; before it in the large round the largest is the triangulation's
            a16(t) + a16(12 t) + 16 + a16(4 x 300) = 19 616 (t = 1 414): 61 552 > 2 x 19 616 and > 2 x 15 344.
  download  small, the largest: the host-pointer search, 4 (nc + 2 np + 8) = 672, and orbx_mappoints_frustum, 5 a16(4 n) + a16(n) = 672.
            large: orbx_sim3_hypotheses, the first call of the large round, a16(4 h) + a16(52 h) + a16(8 h w) = 6 144 (h = 64, w = 5
            mask words) > 2 x 672; then the triangulation's 18 416 > 2 x 6 144.

So each of the three buffers is regrown at least once in the large round, by a request more than twice everything asked of it before,
and the small calls that follow run on buffers far larger than they need."""
import numpy as np
import pytest

import frustum_model as fm
import localmap_scene as ls
import pose_scene as ps
import sim3_scene as s3
import test_mappoints as t_mp
import test_pose_opt as t_pose
import test_sim3 as t_sim3
import test_triangulate as t_tri
from test_projection import _scene as _proj_scene
from test_thread_contexts import _in_thread, _settled

f32 = np.float32
TH, RATIO, WIN_TH, WIN_DIST = 3.0, 0.8, 3.0, 100
SIZES = {
    "small": dict(proj=(64, 48), local=(64, 32, 512), pose=9, tri="one_1", sim3=s3.keys()[1]),        # sim3: 20 points, 5 hypotheses
    "large": dict(proj=(600, 500), local=(300, 600, 1024), pose=257, tri="twenty", sim3=(900, 300, 64, False)),
}
FRAME_KEYS = ("x", "y", "octave", "angle", "u_right", "desc", "bounds")


def _frozen(r):
    """a result in a form that == compares byte for byte"""
    if isinstance(r, dict):
        return tuple((k, _frozen(r[k])) for k in sorted(r))
    if isinstance(r, (tuple, list)):
        return tuple(_frozen(v) for v in r)
    if isinstance(r, np.ndarray):
        return (r.dtype.str, r.shape, r.tobytes())
    return r


def _world(pkg, size):
    """the inputs of every call at one size, and the handles the resident calls read (made here, by the calling thread)"""
    z = SIZES[size]
    w = dict(size=size)
    n_cur, n_pts = z["proj"]
    cur, pts, sf = _proj_scene(700 + n_cur, n_cur, n_pts)
    pts = dict(pts); pts["aux"] = (pts["u"] - 5).astype(f32)
    w.update(cur=cur, pts=pts, sf=sf, df=pkg.DeviceFrame({k: cur[k] for k in FRAME_KEYS}))
    n_feat, n_loc, cap = z["local"]
    frame, geom, desc, has_obs, po = ls.scene(31 + n_feat, n_feat=n_feat, n_pts=n_loc)
    rng = np.random.Generator(np.random.PCG64(n_loc))
    slots = rng.permutation(cap - 12)[:n_loc].astype(np.int32)
    elig = (rng.random(n_loc) < 0.92).astype(np.uint8)
    mp = pkg.MapPoints(cap)
    mp.set(slots, geom, desc)
    w.update(lframe=frame, geom=geom, desc=desc, has_obs=has_obs, pose=po, slots=slots, elig=elig, flags=(elig | (has_obs << 1)).astype(np.uint8),
             cap=cap, mp=mp, ldf=pkg.DeviceFrame({k: frame[k] for k in FRAME_KEYS}))
    sc = t_pose.world(z["pose"], "mixed")[0] if size == "small" else ps.scene(ps.seed_of(z["pose"], "mixed"), z["pose"], "mixed")
    pmp, pslot, _ = t_pose._table(pkg, sc)
    w.update(sc=sc, pdf=pkg.DeviceFrame(t_pose._frame_dict(sc)), pmp=pmp, pslot=pslot)
    s = t_tri._suite(z["tri"])[0]
    w.update(tri=s, tf1=t_tri._device_frame(pkg, s["k1"]), tf2=[t_tri._device_frame(pkg, k) for k in s["k2s"]])
    w["job"] = s3.job(*z["sim3"])
    return w


def _calls(pkg, w):
    """[(name, call)] in the order of the module's docstring: every user of the context, once"""
    m = pkg.ORBmatcher(RATIO, True)
    occ, locc, s, sc = w["cur"]["occupied"], w["lframe"]["occupied"], w["tri"], w["sc"]

    def frame_create():
        return pkg.DeviceFrame({k: w["cur"][k] for k in FRAME_KEYS}).read()

    def mappoints_set():
        mp = pkg.MapPoints(w["cap"])
        mp.set(w["slots"], w["geom"], w["desc"])
        return mp.read(w["slots"])
    return [
        ("search_by_projection_map_points", lambda: m.SearchByProjectionMapPoints(w["cur"], w["pts"], w["sf"], TH)),
        ("frame_create", frame_create),
        ("frame_search_by_projection_map_points", lambda: m.SearchByProjectionMapPointsResident(w["df"], occ, w["pts"], w["sf"], TH)),
        ("frame_window_best", lambda: m.FuseResident(w["df"], w["pts"], w["sf"], None, WIN_TH, WIN_DIST)),
        ("mappoints_set", mappoints_set),
        ("mappoints_frustum", lambda: w["mp"].frustum(w["slots"], w["elig"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.NLEVELS)),
        ("frame_search_local_points", lambda: w["ldf"].search_local_points(locc, w["mp"], w["slots"], w["flags"], w["pose"], ls.CAM, 0.5, ls.LSF,
                                                                            ls.SF, TH, RATIO)),
        ("pose_optimize", lambda: pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])),
        ("frame_pose_optimize", lambda: w["pdf"].pose_optimize(w["pmp"], w["pslot"], ps.INV_SIGMA2, sc["cam"], sc["Tcw"])),
        ("triangulate_pairs", lambda: t_tri._host(pkg, s)),
        ("frame_triangulate", lambda: pkg.frame_triangulate(w["tf1"], s["v1"], w["tf2"], s["v2s"], s["pairs"], s["npairs"], s["sf"], s["sigma2"],
                                                            s["ratio_factor"])),
        ("sim3_hypotheses", lambda: pkg.sim3_hypotheses(w["job"])),
    ]


def _check_small(oracle, w, got):
    """the small results against each module's own model, by that module's own criterion"""
    cur, pts, sf = w["cur"], w["pts"], w["sf"]
    exp, en = oracle.search_by_projection_points(cur, pts, sf, TH, RATIO)
    for name in ("search_by_projection_map_points", "frame_search_by_projection_map_points"):
        assert got[name][1] == en and (got[name][0] == exp).all(), name
    rd = got["frame_create"]
    assert all(rd[k].tobytes() == np.ascontiguousarray(cur[k]).tobytes() for k in FRAME_KEYS[:-1])
    bi, bd, n = got["frame_window_best"]
    ebi, ebd, en = oracle.window_best(cur, pts, sf, None, WIN_TH, 0, WIN_DIST)
    assert n == en and (bi == ebi).all() and (bd == ebd).all()
    g, d = got["mappoints_set"]
    assert g.tobytes() == w["geom"].tobytes() and d.tobytes() == w["desc"].tobytes()
    fr = fm.frustum(w["geom"], w["elig"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    t_mp._same(got["mappoints_frustum"], fr, "frustum")
    lp = dict(u=fr["u"], v=fr["v"], aux=fr["xr"], level=fr["level"], angle=np.zeros(len(w["geom"]), f32), view_cos=fr["view_cos"],
              desc=w["desc"], valid=fr["in_view"], has_obs=w["has_obs"])
    exp, en = oracle.search_by_projection_points(w["lframe"], lp, ls.SF, TH, RATIO)
    match, n, iv = got["frame_search_local_points"]
    assert n == en and (match == exp).all() and iv.tobytes() == fr["in_view"].tobytes()
    sc, model = t_pose.world(SIZES["small"]["pose"], "mixed")
    t_pose.check_against_model(got["pose_optimize"], model, sc["Tcw"], "pose_optimize")
    assert t_pose.same_bytes(got["frame_pose_optimize"], got["pose_optimize"])
    s, exp = t_tri._suite(SIZES["small"]["tri"])
    for name in ("triangulate_pairs", "frame_triangulate"):
        assert t_tri._same(s, got[name], exp) is None, (name, t_tri._same(s, got[name], exp))
    key = SIZES["small"]["sim3"]
    assert t_sim3._diff(got["sim3_hypotheses"], s3.table(*key), key[1]) is None


@pytest.fixture(scope="module")
def worlds(pkg):
    made = _in_thread(lambda: {size: _world(pkg, size) for size in SIZES})   # (the thread's context goes with the thread)
    yield made
    made.clear()


@pytest.mark.gpu
def test_one_family(pkg, worlds):
    """every call sets up, or finds, the one context of its thread; orbx_thread_release gives it back"""
    count = pkg.orbx.debug_thread_contexts
    c0 = count()

    def worker():
        for name, call in _calls(pkg, worlds["small"]):
            call()
            assert count() == c0 + 1, name
        pkg.orbx.thread_release()
        assert count() == c0
    _in_thread(worker)
    assert _settled(pkg, c0) == c0


@pytest.mark.gpu
def test_results_do_not_depend_on_staging_history(pkg, oracle, worlds):
    """expected: each call as the first call of a fresh thread (the small ones also checked against the models).  Then one thread makes
    all the calls small, all of them large in the opposite order, and all of them small again: every result equals its expectation,
    byte for byte.  The sizes, and which request regrows which buffer, are worked out in the module's docstring."""
    c0 = pkg.orbx.debug_thread_contexts()
    first = {size: {name: _in_thread(call) for name, call in _calls(pkg, worlds[size])} for size in SIZES}
    _check_small(oracle, worlds["small"], first["small"])
    expected = {size: {name: _frozen(r) for name, r in first[size].items()} for size in SIZES}

    def worker():
        for size, step in (("small", 1), ("large", -1), ("small", 1)):
            for name, call in _calls(pkg, worlds[size])[::step]:
                assert _frozen(call()) == expected[size][name], (size, name)
    _in_thread(worker)
    assert _settled(pkg, c0) == c0
