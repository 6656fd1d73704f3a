"""orbx_frame_search_local_points: Tracking::SearchLocalPoints' second loop and matcher call (reference src/Tracking.cc:1433-1463) on a
resident frame and a resident map-point table.  The fused call equals orbx_mappoints_frustum followed by
orbx_frame_search_by_projection_map_points, and equals tests/frustum_model.py's points handed to the CPU oracle's map-point search --
with a crowded cluster, where the claim order by has_obs decides who keeps a feature."""
import numpy as np
import pytest

import frustum_model as fm
import localmap_scene as ls

f32 = np.float32


def _frame_only(cur):
    return {k: cur[k] for k in ("x", "y", "octave", "angle", "u_right", "desc", "bounds")}


@pytest.fixture(scope="module")
def world(pkg):
    """one frame of 200 features, a 300-point local map with a cluster of 24, in a table of 512 slots; the model's answer, once"""
    frame, geom, desc, has_obs, po = ls.scene(21, cluster=24)
    rng = np.random.Generator(np.random.PCG64(2))
    slots = rng.permutation(500)[:len(geom)].astype(np.int32)
    elig = (rng.random(len(geom)) < 0.92).astype(np.uint8)
    flags = (elig | (has_obs << 1)).astype(np.uint8)
    mp = pkg.MapPoints(512)
    mp.set(slots, geom, desc)
    df = pkg.DeviceFrame(_frame_only(frame))
    exp = fm.frustum(geom, elig, po, ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    pts = dict(u=exp["u"], v=exp["v"], aux=exp["xr"], level=exp["level"], angle=np.zeros(len(geom), f32), view_cos=exp["view_cos"],
               desc=desc, valid=exp["in_view"], has_obs=has_obs)
    return dict(frame=frame, geom=geom, desc=desc, has_obs=has_obs, pose=po, slots=slots, elig=elig, flags=flags, mp=mp, df=df, exp=exp,
                pts=pts)


@pytest.mark.gpu
@pytest.mark.parametrize("th,ratio", [(1.0, 0.8), (3.0, 0.8), (5.0, 0.6)])
def test_fused_equals_two_calls_and_the_oracle(pkg, oracle, world, th, ratio):
    w = world
    occ = w["frame"]["occupied"]
    got, n, iv = w["df"].search_local_points(occ, w["mp"], w["slots"], w["flags"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, th, ratio)
    # the two calls it fuses
    fr = w["mp"].frustum(w["slots"], w["elig"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    p2 = dict(u=fr["u"], v=fr["v"], aux=fr["xr"], level=fr["level"], view_cos=fr["view_cos"], desc=w["mp"].read(w["slots"])[1],
              valid=fr["in_view"], has_obs=w["has_obs"])
    two, n2 = pkg.ORBmatcher(ratio, True).SearchByProjectionMapPointsResident(w["df"], occ, p2, ls.SF, th)
    assert n == n2 and (got == two).all(), (th, np.nonzero(got != two)[0][:5])
    assert iv.tobytes() == fr["in_view"].tobytes()
    # the model's points through the oracle's search
    exp, en = oracle.search_by_projection_points(w["frame"], w["pts"], ls.SF, th, ratio)
    assert n == en and (got == exp).all(), (th, n, en, np.nonzero(got != exp)[0][:5])
    assert iv.tobytes() == w["exp"]["in_view"].tobytes()
    if th >= 3.0:
        assert n > 40                                                            # the scene matches


@pytest.mark.gpu
def test_claim_order_matters_in_the_cluster(oracle, world):
    """the 24 points of the cluster project onto one feature with look-alike neighbours: with every has_obs bit cleared no point blocks
    a feature and later points overwrite earlier ones -- a different map, which the fused call follows"""
    w = world
    occ = np.zeros(w["df"].n, np.uint8)
    a, na, _ = w["df"].search_local_points(occ, w["mp"], w["slots"], w["flags"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, 5.0, 0.9)
    f0 = (w["flags"] & 1).astype(np.uint8)
    b, nb, _ = w["df"].search_local_points(occ, w["mp"], w["slots"], f0, w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, 5.0, 0.9)
    cur = dict(w["frame"], occupied=occ)
    ea, ena = oracle.search_by_projection_points(cur, w["pts"], ls.SF, 5.0, 0.9)
    eb, enb = oracle.search_by_projection_points(cur, dict(w["pts"], has_obs=np.zeros_like(w["has_obs"])), ls.SF, 5.0, 0.9)
    assert na == ena and (a == ea).all() and nb == enb and (b == eb).all()
    assert (a != b).any()


@pytest.mark.gpu
def test_set_changes_the_next_search_and_empty_calls(pkg, oracle, world):
    w = world
    occ = w["frame"]["occupied"]
    mp = pkg.MapPoints(512)
    mp.set(w["slots"], w["geom"], w["desc"])
    base, nbase, iv0 = w["df"].search_local_points(occ, mp, w["slots"], w["flags"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, 3.0, 0.8)
    i = int(base[base >= 0][0])                                                  # a point that holds a feature
    g2 = w["geom"].copy(); d2 = w["desc"].copy()
    Ow = w["pose"][12:15]
    g2[i, :3] = Ow - (g2[i, :3] - Ow)                                            # ... moves behind the camera
    j = int(base[base >= 0][-1])
    d2[j] = ~d2[j]                                                               # ... and another one's descriptor no longer matches
    mp.set(w["slots"][[i]], g2[[i]], None)
    mp.set(w["slots"][[j]], None, d2[[j]])
    got, n, iv = w["df"].search_local_points(occ, mp, w["slots"], w["flags"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, 3.0, 0.8)
    exp = fm.frustum(g2, w["elig"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.NLEVELS)
    pts = dict(w["pts"], u=exp["u"], v=exp["v"], aux=exp["xr"], level=exp["level"], view_cos=exp["view_cos"], desc=d2, valid=exp["in_view"])
    eg, en = oracle.search_by_projection_points(w["frame"], pts, ls.SF, 3.0, 0.8)
    assert n == en and (got == eg).all() and iv.tobytes() == exp["in_view"].tobytes()
    assert iv0[i] == 1 and iv[i] == 0 and not (got == i).any() and not (got == j).any()
    # no points / no features: ORBX_OK, nothing matched, nothing in view
    e = np.zeros(0, np.int32)
    got, n, iv = w["df"].search_local_points(occ, mp, e, np.zeros(0, np.uint8), w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, 3.0, 0.8)
    assert n == 0 and (got == -1).all() and len(iv) == 0
    empty = pkg.DeviceFrame(dict(x=np.zeros(0, f32), y=np.zeros(0, f32), octave=np.zeros(0, np.int32), angle=np.zeros(0, f32),
                                 u_right=np.zeros(0, f32), desc=np.zeros((0, 32), np.uint8), bounds=(0.0, 0.0, 640.0, 480.0)))
    got, n, iv = empty.search_local_points(None, mp, w["slots"], w["flags"], w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, 3.0, 0.8)
    assert n == 0 and len(got) == 0 and not iv.any()
    # an eligible point whose slot is not set is refused before any launch
    s2 = w["slots"].copy(); s2[0] = 511
    f2 = w["flags"].copy(); f2[0] |= 1
    with pytest.raises(pkg.OrbxError) as ei:
        w["df"].search_local_points(occ, mp, s2, f2, w["pose"], ls.CAM, 0.5, ls.LSF, ls.SF, 3.0, 0.8)
    assert ei.value.code == -1
