"""orbx_pose_optimize, orbx_pose_optimize_batch and orbx_frame_pose_optimize (Optimizer::PoseOptimization, reference
src/Optimizer.cc:286-513) against tests/pose_model.py on the scenes of tests/pose_scene.py.

Exact: n_corr, rounds, n_bad[4], the return value, every flag; Tcw_out == float32(report.pose).  iterations[] is not compared: near
convergence the sign of rho is rounding noise.  The pose and chi2[] are compared in double under a MEASURED bound:

    python tools/pose_spread.py
    SPREAD_POSE = 1.675e-13  SPREAD_CHI2 = 4.848e-14  (x 64: 1.072e-11, 3.103e-12)  scenes to replace: []

is the largest disagreement of the model with itself across its three summation orders over all the scenes below, per pose entry relative
to its block's largest magnitude (rotation block, translation column) and per chi2 relative to max(chi2, 1) (three monocular points are
fitted exactly: their chi2 is rounding residue without relative accuracy, and what a chi2 is compared with is a threshold of 5.991).  The
GPU gets 64 x that spread: it differs from the model in more than the summation order (tree shape, sin / cos, the trial path near
convergence), each rounding noise of that scale, while a real error -- a double invz in the stereo projection, the float rotation used as
a matrix, a wrong restart pose -- is 1e-7 or more.  The scenes' condition (pose_scene.admissible) is asserted here on the model itself, so a
scene that violates it fails loudly instead of hiding a mismatch."""
import ctypes as C

import numpy as np
import pytest

import pose_model as pm
import pose_scene as ps
from tools.pose_spread import ORDERS, chi2_diff, pose_diff

f32 = np.float32
SPREAD_POSE = 1.675e-13          # python tools/pose_spread.py (rounded up in the fourth digit)
SPREAD_CHI2 = 4.848e-14
BOUND_POSE = 64 * SPREAD_POSE    # 1.072e-11
BOUND_CHI2 = 64 * SPREAD_CHI2    # 3.103e-12
assert max(BOUND_POSE, BOUND_CHI2) < 1e-9

CASES = [(n, mix) for n in ps.SIZES for mix in ps.MIXES]
_cache = {}


def world(n, mix, seed=None):
    """a scene and the model's answer (ascending order), computed once"""
    key = (n, mix, seed)
    if key not in _cache:
        sc = ps.scene(ps.seed_of(n, mix) if seed is None else seed, n, mix)
        _cache[key] = (sc, pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], "asc"))
    return _cache[key]


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("Tcw", "outlier", "n_bad", "iterations", "chi2", "pose")) and \
        (a["n_inliers"], a["n_corr"], a["rounds"]) == (b["n_inliers"], b["n_corr"], b["rounds"])


def check_against_model(got, exp, Tcw_in, tag):
    r = exp["rounds"]
    margin = min([float(m.min()) for m in exp["margin"] if len(m)] or [1.0])
    dp = pose_diff(exp["pose"], got["pose"])
    dc = chi2_diff(exp["chi2"], got["chi2"])
    print(f"{tag}: n_corr {got['n_corr']} rounds {got['rounds']} n_bad {list(got['n_bad'])} model {exp['n_bad']} iterations {list(got['iterations'])} model "
          f"{exp['iterations']} margin {margin:.2e} pose {dp:.3e} (bound {BOUND_POSE:.3e}) chi2 {dc:.3e} (bound {BOUND_CHI2:.3e})")
    assert margin >= 1e-6, "the scene has an edge within 1e-6 of its threshold: replace it"
    assert got["n_corr"] == exp["n_corr"] and got["rounds"] == r and list(got["n_bad"]) == exp["n_bad"]
    assert got["n_inliers"] == exp["ret"]
    assert got["outlier"].tobytes() == exp["outlier"].tobytes(), np.nonzero(got["outlier"] != exp["outlier"])[0][:8]
    assert got["Tcw"].tobytes() == np.concatenate([got["pose"].astype(f32), [[0, 0, 0, 1]]]).astype(f32).tobytes() or exp["n_corr"] < 3
    if exp["n_corr"] < 3:
        assert got["Tcw"].tobytes() == np.asarray(Tcw_in, f32).tobytes() and got["n_inliers"] == 0 and not got["outlier"].any()
        assert got["pose"].astype(f32).tobytes() == np.asarray(Tcw_in, f32)[:3].tobytes()
    assert dp <= BOUND_POSE and dc <= BOUND_CHI2


@pytest.mark.gpu
@pytest.mark.parametrize("n,mix", CASES)
def test_matches_the_model(pkg, n, mix):
    sc, exp = world(n, mix)
    rs = [exp] + [pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], o) for o in ORDERS[1:]]
    assert ps.admissible(n, sc, rs), "the scene does not satisfy its condition on the model: replace it (tools/pose_spread.py --select)"
    got = pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])
    check_against_model(got, exp, sc["Tcw"], f"{n} {mix}")
    if n >= 10:
        assert got["rounds"] == 4 and got["outlier"][sc["gross"]].all()      # the point behind the camera among them
    again = pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])
    assert same_bytes(got, again)


def _jobs(count):
    """`count` jobs of unequal sizes, an empty one and one with fewer than 3 correspondences among them (from the second job on)"""
    sizes = [65, 0, 2, 257, 9, 64, 10, 3, 255, 63, 256]
    return [world(sizes[j % len(sizes)], ps.MIXES[j % 3], seed=None if j < len(sizes) else 70000 + j)[0] for j in range(count)]


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 7, 33])
def test_batch_equals_the_single_calls(pkg, count):
    scs = _jobs(count)
    got = pkg.pose_optimize_batch([(sc["obs"], sc["cam"], sc["Tcw"]) for sc in scs])
    assert len(got) == count
    for j, sc in enumerate(scs):
        key = ("single", id(sc))
        if key not in _cache:
            _cache[key] = pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])
        assert same_bytes(got[j], _cache[key]), j


@pytest.mark.gpu
def test_three_unequal_jobs_in_one_batch(pkg):
    """sizes that are no multiple of the 16 bytes the staging pads to, an empty job between them: every job's arrays lie where its own
    sizes put them"""
    scs = [ps.scene(81000 + n, n, mix) for n, mix in ((33, "mixed"), (0, "mono"), (100, "stereo"))]
    scs[1]["obs"] = {k: v[:0] for k, v in scs[1]["obs"].items()}                        # n = 0: no feature at all
    assert [len(sc["obs"]["x"]) for sc in scs] == [52, 0, 153]
    got = pkg.pose_optimize_batch([(sc["obs"], sc["cam"], sc["Tcw"]) for sc in scs])
    assert len(got) == 3 and got[1]["n_corr"] == 0 and got[0]["n_corr"] > 3 and got[2]["n_corr"] > 3
    for j, sc in enumerate(scs):
        assert same_bytes(got[j], pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])), j


def _frame_dict(sc):
    n = len(sc["octave"])
    rng = np.random.Generator(np.random.PCG64(n))
    o = sc["obs"]
    return dict(x=o["x"], y=o["y"], octave=sc["octave"], angle=rng.uniform(0, 360, n).astype(f32), u_right=o["u_right"],
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), bounds=(0.0, 0.0, float(ps.W), float(ps.H)))


def _table(pkg, sc, capacity=2048, seed=5):
    """the scene's points in a table: -> MapPoints, slot_of_feature, geom"""
    has = sc["obs"]["has_point"].astype(bool)
    n = len(has)
    rng = np.random.Generator(np.random.PCG64(seed))
    slot = np.full(n, -1, np.int32)
    slot[has] = rng.permutation(capacity - 8)[:int(has.sum())]
    geom = np.zeros((int(has.sum()), 8), f32)
    geom[:, :3] = sc["obs"]["Xw"][has]
    geom[:, 3:] = rng.uniform(0.5, 2.0, (len(geom), 5))
    mp = pkg.MapPoints(capacity)
    if len(geom):
        mp.set(slot[has], geom, rng.integers(0, 256, (len(geom), 32), dtype=np.uint8))
    return mp, slot, geom


@pytest.mark.gpu
@pytest.mark.parametrize("n,mix", [(257, "mixed"), (64, "mono"), (2, "stereo"), (0, "mixed")])
def test_resident_equals_host_pointers(pkg, n, mix):
    sc, exp = world(n, mix)
    host = pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])
    df = pkg.DeviceFrame(_frame_dict(sc))
    mp, slot, _ = _table(pkg, sc)
    got = df.pose_optimize(mp, slot, ps.INV_SIGMA2, sc["cam"], sc["Tcw"])
    assert same_bytes(got, host)
    assert same_bytes(df.pose_optimize(mp, slot, ps.INV_SIGMA2, sc["cam"], sc["Tcw"]), host)


@pytest.mark.gpu
def test_resident_after_a_set_on_another_stream(pkg):
    """three points move through orbx_mappoints_set on a stream of the caller's; the next optimisation, on the library's stream, sees them"""
    import torch
    sc, _ = world(255, "mixed")
    df = pkg.DeviceFrame(_frame_dict(sc))
    mp, slot, geom = _table(pkg, sc)
    before = df.pose_optimize(mp, slot, ps.INV_SIGMA2, sc["cam"], sc["Tcw"])
    has = np.nonzero(sc["obs"]["has_point"])[0]
    inl = [k for k in range(len(has)) if not before["outlier"][has[k]]][:3]
    g2 = geom.copy()
    g2[inl, :3] += f32(0.25)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    mp.set(slot[has[inl]], g2[inl], None, stream=stream.cuda_stream)
    got = df.pose_optimize(mp, slot, ps.INV_SIGMA2, sc["cam"], sc["Tcw"])
    obs2 = dict(sc["obs"], Xw=sc["obs"]["Xw"].copy())
    obs2["Xw"][has[inl]] = g2[inl, :3]
    host = pkg.pose_optimize(obs2, sc["cam"], sc["Tcw"])
    assert same_bytes(got, host) and not same_bytes(got, before)
    stream.synchronize()


@pytest.mark.gpu
def test_resident_on_a_frame_from_extraction(pkg):
    import torch
    sc, _ = world(65, "mixed")
    o = sc["obs"]
    n, cap = len(sc["octave"]), 128
    k = np.zeros((2, cap), pkg.KP_DTYPE)
    k["x"][1, :n] = o["x"]; k["y"][1, :n] = o["y"]; k["octave"][1, :n] = sc["octave"]; k["size"][1, :n] = 31
    u = np.full((2, cap), 55.5, f32); u[1, :n] = o["u_right"]
    d = np.zeros((2, cap, 32), np.uint8)
    cnt = np.array([cap // 3, n], np.int32)
    dev = torch.device("cuda", 0)
    tk, td, tu, tn = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev) for a in (k, d, u, cnt)]
    torch.cuda.synchronize()
    df = pkg.DeviceFrame.from_extraction(0, tk.data_ptr(), td.data_ptr(), tn.data_ptr(), cap, 1, d_u_right=tu.data_ptr() + 4 * cap,
                                         bounds=(0.0, 0.0, float(ps.W), float(ps.H)))
    mp, slot, _ = _table(pkg, sc)
    got = df.pose_optimize(mp, slot, ps.INV_SIGMA2, sc["cam"], sc["Tcw"])       # the first call on the frame: it waits for the creation
    assert same_bytes(got, pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"]))
    # the octaves of such a frame are on the device only: the kernel checks them before it optimises
    with pytest.raises(pkg.OrbxError) as ei:
        df.pose_optimize(mp, slot, ps.INV_SIGMA2[:int(sc["octave"][sc["obs"]["has_point"] > 0].max())], sc["cam"], sc["Tcw"])
    assert ei.value.code == -1 and "octave" in str(ei.value)


def chain_inputs(oracle_match, ls, frame, slots):
    """match_cur (an index into slots, -1 none) -> slot_of_feature"""
    return np.where(oracle_match >= 0, slots[np.maximum(oracle_match, 0)], -1).astype(np.int32)


def chain_world(ls):
    frame, geom, desc, has_obs, po = ls.scene(21)
    rng = np.random.Generator(np.random.PCG64(2))
    slots = rng.permutation(500)[:len(geom)].astype(np.int32)
    flags = (np.ones(len(geom), np.uint8) | (has_obs << 1)).astype(np.uint8)
    Tcw = np.eye(4, dtype=f32)
    Tcw[:3, :3] = po[:9].reshape(3, 3); Tcw[:3, 3] = po[9:12]
    isig = (1.0 / (ls.SF.astype(np.float64) ** 2)).astype(f32)
    return frame, geom, desc, slots, flags, po, Tcw, isig


def chain_obs(fr, g, slot, isig):
    """the model's input from what orbx_frame_read / orbx_mappoints_read give back"""
    has = (slot >= 0).astype(np.uint8)
    Xw = np.zeros((len(slot), 3), f32)
    Xw[slot >= 0] = g[:, :3]
    return dict(x=fr["x"], y=fr["y"], u_right=fr["u_right"], inv_sigma2=isig[fr["octave"]], Xw=Xw, has_point=has)


@pytest.mark.gpu
def test_chain_search_then_optimise(pkg):
    """orbx_frame_search_local_points -> match_cur -> slot_of_feature -> orbx_frame_pose_optimize, nothing but slots and the pose in between"""
    import localmap_scene as ls
    frame, geom, desc, slots, flags, po, Tcw, isig = chain_world(ls)
    mp = pkg.MapPoints(512)
    mp.set(slots, geom, desc)
    df = pkg.DeviceFrame({k: frame[k] for k in ("x", "y", "octave", "angle", "u_right", "desc", "bounds")})
    match, nm, _ = df.search_local_points(None, mp, slots, flags, po, ls.CAM, 0.5, ls.LSF, ls.SF, 3.0, 0.8)
    assert nm > 40
    slot = chain_inputs(match, ls, frame, slots)
    got = df.pose_optimize(mp, slot, isig, ls.CAM[:5], Tcw)
    obs = chain_obs(df.read(), mp.read(slot[slot >= 0])[0], slot, isig)
    rs = [pm.optimize(obs, ls.CAM[:5], Tcw, o) for o in ORDERS]
    assert ps.admissible(0, dict(gross=np.zeros(len(slot), bool)), rs), "the chain's scene does not satisfy its condition on the model"
    assert max(pose_diff(rs[0]["pose"], r["pose"]) for r in rs[1:]) <= SPREAD_POSE
    check_against_model(got, rs[0], Tcw, "chain")
    assert got["n_corr"] == int((match >= 0).sum()) and got["rounds"] == 4


@pytest.mark.gpu
def test_refusals(pkg):
    L = pkg.lib()
    sc, _ = world(10, "mixed")
    po, keep = pkg.orbx._pose_obs(sc["obs"], "test")
    cam = np.ascontiguousarray(sc["cam"], f32); T = np.ascontiguousarray(sc["Tcw"], f32).reshape(-1)
    out = np.zeros(16, f32); fl = np.zeros(po.n, np.uint8); ni = C.c_int()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda obs, cam_=cam, T_=T, out_=out, fl_=fl, ni_=ni: L.orbx_pose_optimize(
        0, None if obs is None else C.byref(obs), None if cam_ is None else p(cam_), None if T_ is None else p(T_),
        None if out_ is None else p(out_), None if fl_ is None else p(fl_), None if ni_ is None else C.byref(ni_), None)
    assert call(po) == 0                                                         # the arguments are good (report NULL)
    assert call(None) == -1 and call(po, cam_=None) == -1 and call(po, T_=None) == -1 and call(po, out_=None) == -1
    assert call(po, fl_=None) == -1 and call(po, ni_=None) == -1
    for field in ("x", "y", "u_right", "inv_sigma2", "Xw", "has_point"):
        bad = pkg.orbx.PoseObs.from_buffer_copy(po)
        setattr(bad, field, None)
        assert call(bad) == -1, field
    for n in (-1, 65536):
        bad = pkg.orbx.PoseObs.from_buffer_copy(po)
        bad.n = n
        assert call(bad) == -1, n
    # the batch: njobs outside [1, 1024], a bad job
    jobs = (pkg.orbx.PoseJob * 2)()
    for j in range(2):
        jobs[j].obs = C.pointer(po); jobs[j].cam = p(cam); jobs[j].Tcw = p(T); jobs[j].Tcw_out = p(out); jobs[j].outlier = p(fl)
    assert L.orbx_pose_optimize_batch(0, jobs, 2) == 0
    assert L.orbx_pose_optimize_batch(0, jobs, 0) == -1 and L.orbx_pose_optimize_batch(0, jobs, 1025) == -1
    assert L.orbx_pose_optimize_batch(0, None, 1) == -1
    jobs[1].cam = None
    assert L.orbx_pose_optimize_batch(0, jobs, 2) == -1
    # the resident form
    df = pkg.DeviceFrame(_frame_dict(sc))
    mp, slot, _ = _table(pkg, sc, capacity=64)
    res = lambda f=df._h, m=mp._h, s=slot, isig=ps.INV_SIGMA2, nl=ps.NLEVELS, cam_=cam, T_=T, out_=out, fl_=fl, ni_=ni: \
        L.orbx_frame_pose_optimize(f, m, None if s is None else p(s), None if isig is None else p(isig), nl, None if cam_ is None else p(cam_),
                                   None if T_ is None else p(T_), None if out_ is None else p(out_), None if fl_ is None else p(fl_),
                                   None if ni_ is None else C.byref(ni_), None)
    assert res() == 0
    assert res(f=None) == -1 and res(m=None) == -1 and res(s=None) == -1 and res(isig=None) == -1 and res(cam_=None) == -1
    assert res(T_=None) == -1 and res(out_=None) == -1 and res(fl_=None) == -1 and res(ni_=None) == -1
    assert res(nl=0) == -1 and res(nl=17) == -1
    i = int(np.nonzero(slot >= 0)[0][0])
    for v in (64, -2, 63):                                                       # beyond the capacity, below -1, in range but never set
        s2 = slot.copy(); s2[i] = v
        assert res(s=s2) == -1, v
    assert "not set" in L.orbx_last_error().decode()
    # an octave outside [0, nlevels): a frame made from host pointers is refused before any device work
    nl = int(sc["octave"][slot >= 0].max())
    assert res(nl=nl) == -1 and "octave" in L.orbx_last_error().decode()
    big = np.zeros(65536, f32)                                                   # n outside [0, 65535] cannot become a frame at all
    with pytest.raises(pkg.OrbxError):
        pkg.DeviceFrame(dict(x=big, y=big, octave=np.zeros(65536, np.int32), angle=big, u_right=big, desc=np.zeros((65536, 32), np.uint8),
                             bounds=(0.0, 0.0, 10.0, 10.0)))
    import torch
    if torch.cuda.device_count() >= 2:                                           # a frame and a table on different devices
        mp1 = pkg.MapPoints(64, device=1)
        assert res(m=mp1._h) == -1 and "different devices" in L.orbx_last_error().decode()
