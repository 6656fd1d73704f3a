"""orbx_mapgraph_refresh_points (include/orbx.h) -- MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors from the resident graph,
the resident keyframes and the map-point table -- against the sequential model of tests/refresh_model.py.  Every operation of the call is
specified, so every comparison is on equal bytes (NaN equal to NaN): outputs, table slots read back, and the pattern a row keeps when it
is not updated.  CPU: the ABI surface."""
import os

import numpy as np
import pytest

from refresh_scenes import PATTERN, SCALE_FACTORS, Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM, DESC = 1, 2


def test_symbol_exported_and_typed(pkg):
    import __graft_entry__ as ge
    ge.build()
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    assert "orbx_mapgraph_refresh_points(" in hdr and "ORBX_REFRESH_GEOM 1" in hdr and "ORBX_REFRESH_DESC 2" in hdr
    assert pkg.lib().orbx_mapgraph_refresh_points.argtypes is not None
    assert callable(pkg.MapGraph.refresh_points) and (pkg.REFRESH_GEOM, pkg.REFRESH_DESC) == (1, 2)


# ------------------------------------------------------------------------------------------------ helpers

def device(pkg, sc, order="forward", extras=False, limits=None):
    g = pkg.MapGraph(*(limits or sc.limits))
    sc.apply(g, order, extras)
    return g, [pkg.DeviceFrame(sc.frame(k)) for k in range(sc.n_kf)]


def filled_table(pkg, sc, capacity, slots):
    """a table whose listed slots hold the scene's positions and otherwise recognisable values"""
    t = pkg.MapPoints(capacity)
    r = np.random.RandomState(3)
    geom = r.rand(len(slots), 8).astype(np.float32) + np.float32(100.0)
    geom[:, :3] = sc.pos[:len(slots)]
    desc = r.randint(0, 256, (len(slots), 32)).astype(np.uint8)
    t.set(slots, geom, desc)
    return t, geom, desc


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def check_outputs(res, want, tag=""):
    """the model's rows where a bit is set, the pattern where it is clear"""
    pat32 = np.full(8, PATTERN, np.uint8).view(np.float32)[0]
    pati = np.full(4, PATTERN, np.uint8).view(np.int32)[0]
    for i, w in enumerate(want):
        assert res.status[i] == w["status"], (tag, i, "status", res.status[i], w["status"])
        if w["status"] & GEOM:
            assert same(res.geom[i], w["geom"]), (tag, i, "geom", res.geom[i], w["geom"])
        else:
            assert (res.geom[i].view(np.uint8) == PATTERN).all(), (tag, i, "geom written", pat32)
        if w["status"] & DESC:
            assert (res.best_kf[i], res.best_idx[i]) == (w["best_kf"], w["best_idx"]), (tag, i, "winner", res.best_kf[i], res.best_idx[i], w)
            assert same(res.desc[i], w["desc"]), (tag, i, "desc")
        else:
            assert res.best_kf[i] == pati and res.best_idx[i] == pati and (res.desc[i] == PATTERN).all(), (tag, i, "descriptor written")


def check_table(table, slots, want, geom0, desc0, tag=""):
    tg, td = table.read(slots)
    for i, w in enumerate(want):
        assert same(tg[i], w["geom"] if w["status"] & GEOM else geom0[i]), (tag, i, "table geom", tg[i])
        assert same(td[i], w["desc"] if w["status"] & DESC else desc0[i]), (tag, i, "table desc")
    return tg, td


def run(pkg, g, sc, frames, pts, what, table=None, bad=(), **kw):
    kw.setdefault("pos", sc.pos[pts])
    kw.setdefault("ref_kf", sc.ref_kf[pts])
    kw.setdefault("keyframes", sc.keyframes(frames, bad))
    kw.setdefault("scale_factors", SCALE_FACTORS)
    return g.refresh_points(pts, table=table, what=what, out=pkg.RefreshResult(len(pts), PATTERN), **kw)


def same_result(a, b):
    return all(same(getattr(a, k), getattr(b, k)) for k in ("status", "geom", "best_kf", "best_idx", "desc"))


@pytest.fixture(scope="module")
def small(pkg):
    sc = Scene(5, 6, 40, 60, 8)
    g, frames = device(pkg, sc)
    return sc, sc.model(), g, frames


# ------------------------------------------------------------------------------------------------ 1. a random small map

@pytest.mark.gpu
@pytest.mark.parametrize("what", [GEOM, DESC, GEOM | DESC])
def test_random_small_map(pkg, small, what):
    sc, sg, g, frames = small
    pts = np.random.RandomState(1).permutation(sc.n_pts).astype(np.int32)
    want = sc.expect(sg, pts.tolist(), what)
    assert sum(1 for w in want if w["status"] == what) == len(pts)
    bare = run(pkg, g, sc, frames, pts, what)                                  # no table
    check_outputs(bare, want, "no table")
    t1, g1, d1 = filled_table(pkg, sc, 64, np.arange(60, dtype=np.int32))
    r1 = run(pkg, g, sc, frames, pts, what, table=t1)                          # pos given, the table's slots are the points'
    check_outputs(r1, want, "pos given")
    check_table(t1, pts, want, g1[pts], d1[pts], "pos given")
    slots2 = (63 - pts).astype(np.int32)
    t2 = pkg.MapPoints(64)
    t2.set(slots2, g1[pts], d1[pts])
    r2 = run(pkg, g, sc, frames, pts, what, table=t2, table_slots=slots2, pos=None)   # X Y Z as the table holds them
    assert same_result(r1, r2) and same_result(r1, bare)
    check_table(t2, slots2, want, g1[pts], d1[pts], "pos from the table")


# ------------------------------------------------------------------------------------------------ 2. the stored order of a row

@pytest.mark.gpu
@pytest.mark.parametrize("order,extras", [("reversed", False), ("shuffled", True)])
def test_order_independence(pkg, small, order, extras):
    sc, sg, g, frames = small
    pts = np.arange(sc.n_pts, dtype=np.int32)
    g2, _ = device(pkg, sc, order, extras)
    assert g2.read_points() == g.read_points()
    want = sc.expect(sg, pts.tolist(), 3)
    ta, ga, da = filled_table(pkg, sc, 60, pts)
    tb, _, _ = filled_table(pkg, sc, 60, pts)
    ra = run(pkg, g, sc, frames, pts, 3, table=ta)
    rb = run(pkg, g2, sc, frames, pts, 3, table=tb)
    check_outputs(rb, want, order)
    assert same_result(ra, rb)
    assert all(same(x, y) for x, y in zip(ta.read(pts), tb.read(pts)))


# ------------------------------------------------------------------------------------------------ 3. long rows

@pytest.mark.gpu
@pytest.mark.parametrize("bad", [(), tuple(range(0, 256, 7))])
def test_long_rows(pkg, bad):
    """rows of 65 and 200 observers (beyond a wave), of 64 exactly, and of max_obs = 256: the row that fills the kernel's LDS arrays to
    their last entry and asks for the largest dynamic LDS a launch can need (56 * 256 + 2 * 256^2 = 145 408 bytes)"""
    r = np.random.RandomState(4)
    rows = {p: [(int(k), int(r.randint(0, 4))) for k in r.permutation(256)[:n]] for p, n in enumerate((65, 200, 64, 3, 256))}
    sc = Scene(6, 256, 4, 5, 256, rows=rows)
    g, frames = device(pkg, sc, "reversed")
    pts = np.arange(5, dtype=np.int32)
    want = sc.expect(sc.model(), pts.tolist(), 3, bad=set(bad))
    t, g0, d0 = filled_table(pkg, sc, 5, pts)
    res = run(pkg, g, sc, frames, pts, 3, table=t, bad=set(bad))
    check_outputs(res, want, "long rows")
    check_table(t, pts, want, g0, d0, "long rows")
    assert [w["status"] for w in want] == [3, 3, 3, 3, 3]
    # the longest row decides the launch's LDS: the rows of 65 and 64 alone take another size, and give the same bytes
    short = run(pkg, g, sc, frames, pts[[0, 2]], 3, bad=set(bad))
    check_outputs(short, [want[0], want[2]], "long rows, a short launch")


# ------------------------------------------------------------------------------------------------ 4. ties

@pytest.mark.gpu
def test_ties_go_to_the_lowest_slot(pkg):
    rows = {0: [(7, 1), (5, 0), (3, 1), (1, 0)], 1: [(6, 0), (4, 1), (2, 0), (0, 1)]}
    sc = Scene(8, 8, 2, 2, 8, rows=rows)
    A, B = sc.desc[3, 1].copy(), sc.desc[2, 0].copy()
    sc.desc[5, 0] = A; sc.desc[1, 0] = ~A; sc.desc[7, 1] = A ^ np.uint8(0xF0)     # medians 256/128 apart: slots 3 and 5 tie at 0
    sc.desc[4, 1] = B; sc.desc[6, 0] = B; sc.desc[0, 1] = ~B                      # slots 2, 4 and 6 tie at 0, slot 0 does not
    g, frames = device(pkg, sc)                                                  # rows stored in descending slot order
    pts = np.array([0, 1], np.int32)
    want = sc.expect(sc.model(), [0, 1], DESC)
    res = run(pkg, g, sc, frames, pts, DESC)
    check_outputs(res, want, "ties")
    assert res.best_kf.tolist() == [3, 2] and res.best_idx.tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ 5. bad keyframes

@pytest.mark.gpu
def test_bad_keyframes(pkg):
    sc = Scene(9, 6, 40, 60, 8)
    sc.rows[0] = [(1, 3), (4, 5)]; sc.ref_kf[0] = 1                     # every observer will be bad
    sc.rows[1] = [(0, 2), (2, 7), (3, 9), (5, 1)]; sc.ref_kf[1] = 3     # (2, 7) will outlive keyframe 2
    sc.matches = {key: (-1 if p in (0, 1) else p) for key, p in sc.matches.items()}   # no match names the two: nothing erases their rows
    sc.matches[(2, 7)] = -1
    sc.ref_kf[sc.ref_kf == 2] = 3
    g, frames = device(pkg, sc)
    sg = sc.model()
    for x in (g, sg):
        x.erase_keyframe(2)
    assert g.read_points() == {p: v for p, v in sg.dump()[1].items()}
    assert (2, 7) in g.read_point(1)["obs"] and g.read_keyframe(2) is None
    bad = {1, 4, 2}
    pts = np.arange(sc.n_pts, dtype=np.int32)
    want = sc.expect(sg, pts.tolist(), 3, bad=bad)
    assert want[0]["status"] == GEOM and want[1]["status"] == 3
    assert any(w["status"] == 0 for w in want)                          # the erasure made some points bad
    t, g0, d0 = filled_table(pkg, sc, 60, pts)
    kfd = sc.keyframes(frames, bad)
    kfd["frame"] = [None if b else f for b, f in zip(kfd["bad"], kfd["frame"])]   # a bad keyframe needs no frame
    res = run(pkg, g, sc, frames, pts, 3, table=t, keyframes=kfd)
    check_outputs(res, want, "bad keyframes")
    check_table(t, pts, want, g0, d0, "bad keyframes")


# ------------------------------------------------------------------------------------------------ 6. the reference keyframe outside the row

@pytest.mark.gpu
def test_reference_keyframe_not_in_the_row(pkg, small):
    sc, sg, g, frames = small
    ref = sc.ref_kf.copy()
    moved = 0
    for p in range(sc.n_pts):
        free = [k for k in range(sc.n_kf) if k not in {k for k, _ in sc.rows[p]}]
        if free:
            ref[p] = free[p % len(free)]
            moved += 1
    assert moved > 20
    pts = np.arange(sc.n_pts, dtype=np.int32)
    want = sc.expect(sg, pts.tolist(), GEOM, ref_kf=ref)
    res = run(pkg, g, sc, frames, pts, GEOM, ref_kf=ref)
    check_outputs(res, want, "ref outside the row")
    p = next(p for p in range(sc.n_pts) if ref[p] != sc.ref_kf[p])
    d = np.float32(np.sqrt(np.sum((sc.pos[p].astype(np.float64) - sc.centre[ref[p]].astype(np.float64)) ** 2)))
    assert abs(res.geom[p, 7] / (d * SCALE_FACTORS[sc.octave[ref[p], 0]]) - 1) < 1e-5   # feature 0's octave


# ------------------------------------------------------------------------------------------------ 7. points that return early

@pytest.mark.gpu
def test_dead_and_bad_points(pkg):
    sc = Scene(10, 6, 40, 60, 8)
    for p in range(50, 60):
        del sc.rows[p]                                                   # slots that never were points
    g, frames = device(pkg, sc)
    sg = sc.model()
    for x in (g, sg):
        x.erase_points([5, 9, 20])
    # (a live point with an empty row cannot be made: the erasure that empties a row leaves nObs <= 2 and makes the point bad)
    pts = np.array([5, 55, 2, 9, 59, 20, 7], np.int32)
    want = sc.expect(sg, pts.tolist(), 3)
    assert [w["status"] for w in want] == [0, 0, 3, 0, 0, 0, 3]
    t, g0, d0 = filled_table(pkg, sc, 60, np.arange(60, dtype=np.int32))
    before = t.read(pts)
    res = run(pkg, g, sc, frames, pts, 3, table=t, pos=None)
    check_outputs(res, want, "early returns")
    after = t.read(pts)
    for i in (0, 1, 3, 4, 5):
        assert before[0][i].tobytes() == after[0][i].tobytes() and before[1][i].tobytes() == after[1][i].tobytes(), i
    # nothing but dead points: no launch, status 0
    res = run(pkg, g, sc, frames, pts[[0, 1]], 3, table=t)
    assert res.status.tolist() == [0, 0] and (res.desc == PATTERN).all()


# ------------------------------------------------------------------------------------------------ 8. zero distances

@pytest.mark.gpu
def test_degenerate_positions(pkg, small):
    sc, sg, g, frames = small
    pos = sc.pos.copy()
    p_nan = next(p for p in range(sc.n_pts) if len(sc.rows[p]) >= 2)
    other = next(k for k, _ in sc.rows[p_nan] if k != sc.ref_kf[p_nan])
    pos[p_nan] = sc.centre[other]                                        # P == Ow of an observer: 0 * inf
    p_zero = p_nan + 1
    pos[p_zero] = sc.centre[sc.ref_kf[p_zero]]                           # P == Ow of the reference keyframe
    pts = np.arange(sc.n_pts, dtype=np.int32)
    want = sc.expect(sg, pts.tolist(), GEOM, pos=pos)
    res = run(pkg, g, sc, frames, pts, GEOM, pos=pos)
    check_outputs(res, want, "degenerate")
    assert np.isnan(res.geom[p_nan, 4:7]).all() and np.isfinite(res.geom[p_nan, [3, 7]]).all()
    assert res.geom[p_zero, 3] == 0.0 and res.geom[p_zero, 7] == 0.0


# ------------------------------------------------------------------------------------------------ 9. the table as the searches read it

@pytest.mark.gpu
def test_frustum_on_the_refreshed_table(pkg, small):
    sc, sg, g, frames = small
    pts = np.arange(sc.n_pts, dtype=np.int32)
    want = sc.expect(sg, pts.tolist(), 3)
    ta = pkg.MapPoints(60)
    res = run(pkg, g, sc, frames, pts, 3, table=ta)                      # a table that had nothing: both halves given by the call
    assert (res.status == 3).all()
    tb = pkg.MapPoints(60)
    tb.set(pts, np.stack([w["geom"] for w in want]), np.stack([w["desc"] for w in want]))
    pose = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 6, 0, 0, -6], np.float32)
    cam = np.array([500, 500, 320, 240, 40, 0, 0, 640, 480], np.float32)
    el = np.ones(len(pts), np.uint8)
    fa = ta.frustum(pts, el, pose, cam, 0.5, float(np.log(np.float32(1.2))), 8)
    fb = tb.frustum(pts, el, pose, cam, 0.5, float(np.log(np.float32(1.2))), 8)
    assert fb["in_view"].sum() > 10
    for k in fa:
        assert same(fa[k], fb[k]), k
    assert all(same(x, y) for x, y in zip(ta.read(pts), tb.read(pts)))


# ------------------------------------------------------------------------------------------------ 10. refusals

@pytest.fixture(scope="module")
def roomy(pkg):
    """the small map in a graph with two more keyframe slots: 6 in use and never listed, 7 free"""
    sc = Scene(5, 6, 40, 60, 8)
    g, frames = device(pkg, sc, limits=(8, 40, 64, 8))
    g.set_keyframe(6, sc.octave[0], np.zeros(40, np.uint8), np.zeros(40, np.uint8))
    tiny = pkg.DeviceFrame({k: (v[:1] if k != "bounds" else v) for k, v in sc.frame(0).items()})
    t, g0, d0 = filled_table(pkg, sc, 64, np.arange(60, dtype=np.int32))
    return sc, g, frames, tiny, t


def with_extra_keyframe(sc, frames, slot):
    kfd = sc.keyframes(frames)
    return dict(slot=np.append(kfd["slot"], np.int32(slot)), centre=np.vstack([kfd["centre"], [[0, 0, 0]]]).astype(np.float32),
                bad=np.append(kfd["bad"], np.uint8(0)), frame=kfd["frame"] + [None])


def twice(kfd):
    return dict(slot=np.append(kfd["slot"], kfd["slot"][0]), centre=np.vstack([kfd["centre"], kfd["centre"][:1]]),
                bad=np.append(kfd["bad"], np.uint8(0)), frame=kfd["frame"] + [kfd["frame"][0]])


P10 = np.arange(10, dtype=np.int32)
REFUSALS = [
    ("what 0", -1, lambda sc, fr, tiny: dict(what=0)),
    ("what 4", -1, lambda sc, fr, tiny: dict(what=4)),
    ("negative point slot", -1, lambda sc, fr, tiny: dict(points=np.array([0, -1, 2], np.int32))),
    ("point slot twice", -1, lambda sc, fr, tiny: dict(points=np.array([0, 3, 0], np.int32))),
    ("point slot beyond max_points", -2, lambda sc, fr, tiny: dict(points=np.array([0, 64, 2], np.int32))),
    ("negative keyframe slot", -1, lambda sc, fr, tiny: dict(keyframes=with_extra_keyframe(sc, fr, -1))),
    ("keyframe slot twice", -1, lambda sc, fr, tiny: dict(keyframes=twice(sc.keyframes(fr)))),
    ("keyframe slot beyond max_keyframes", -2, lambda sc, fr, tiny: dict(keyframes=with_extra_keyframe(sc, fr, 8))),
    ("negative table slot", -1, lambda sc, fr, tiny: dict(table_slots=np.where(P10 == 4, -1, P10).astype(np.int32))),
    ("table slot twice", -1, lambda sc, fr, tiny: dict(table_slots=np.where(P10 == 4, 5, P10).astype(np.int32))),
    ("table slot beyond the capacity", -2, lambda sc, fr, tiny: dict(table_slots=np.where(P10 == 4, 64, P10).astype(np.int32))),
    ("a row names a keyframe that is not listed", -1, lambda sc, fr, tiny: dict(keyframes=sc.keyframes(fr, slots=[1, 2, 3, 4, 5]))),
    ("ref_kf not listed", -1, lambda sc, fr, tiny: dict(ref_kf=np.where(P10 == 2, 6, sc.ref_kf[:10]).astype(np.int32))),
    ("ref_kf not in use", -1, lambda sc, fr, tiny: dict(ref_kf=np.where(P10 == 2, 7, sc.ref_kf[:10]).astype(np.int32),
                                                        keyframes=with_extra_keyframe(sc, fr, 7))),
    ("ref_kf missing", -1, lambda sc, fr, tiny: dict(ref_kf=None)),
    ("octave beyond nlevels", -1, lambda sc, fr, tiny: dict(scale_factors=SCALE_FACTORS[:1])),
    ("pos missing, the slot never had its geometry", -1, lambda sc, fr, tiny: dict(pos=None, table_slots=(P10 + 50).astype(np.int32), fresh=True)),
    ("pos missing, no table", -1, lambda sc, fr, tiny: dict(pos=None, table=None)),
    ("a keyframe that is not bad without a frame", -1, lambda sc, fr, tiny: dict(keyframes=sc.keyframes([None] * 6))),
    ("a frame with fewer features than the row's index", -1, lambda sc, fr, tiny: dict(keyframes=sc.keyframes([tiny] + fr[1:]))),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,code,change", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals(pkg, roomy, name, code, change):
    sc, g, frames, tiny, table = roomy
    kw = dict(points=P10, what=3, table=table, table_slots=None, pos=sc.pos[:10], ref_kf=sc.ref_kf[:10], keyframes=sc.keyframes(frames),
              scale_factors=SCALE_FACTORS)
    kw.update(change(sc, frames, tiny))
    if kw.pop("fresh", False):
        kw["table"] = table = pkg.MapPoints(64)
        table.set(P10, np.zeros((10, 8), np.float32), np.zeros((10, 32), np.uint8))    # other slots: the listed ones have nothing
    pts = kw.pop("points")
    if len(pts) != 10:
        kw["pos"], kw["ref_kf"] = (None if kw["pos"] is None else kw["pos"][:len(pts)]), kw["ref_kf"][:len(pts)]
    graph_before = g.read_points()
    every = np.arange(64, dtype=np.int32)
    table_before = None if table is None else table.read(every)
    out = pkg.RefreshResult(len(pts), PATTERN)
    with pytest.raises(pkg.OrbxError) as e:
        g.refresh_points(pts, out=out, **kw)
    assert e.value.code == code, (name, str(e.value))
    assert g.read_points() == graph_before
    if table is not None:
        assert all(same(x, y) for x, y in zip(table.read(every), table_before))
    for a in (out.status, out.geom, out.best_kf, out.best_idx, out.desc):
        assert (a.view(np.uint8) == PATTERN).all(), name
    # and the call is still good for the same arguments without the fault
    if name == "what 0":
        res = run(pkg, g, sc, frames, P10, 3, table=table)
        assert (res.status == 3).all()
