"""Resident current frame (include/orbx.h: orbx_frame): the frame Tracking searches by projection two to four times per tracked frame
(reference src/Tracking.cc:1065,:1072,:1463,:1763,:1777) uploaded once -- or taken straight from the extraction's device buffers -- with
its 64x48 grid (src/Frame.cc:261-279) built once; the searches move only the points and the per-call `occupied` bytes.
CPU: the ABI surface and its refusals.  GPU: every resident search equals its host-pointer twin and the CPU oracle on ONE reused frame,
also while `occupied` changes between calls; frames made from extraction buffers equal those buffers bit for bit (with on-device
undistortion equal to orbx_undistort_keypoints) and survive the buffers being overwritten; the adaptor cache (adapter/ORBmatcher_proj.cc)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_projection import _scene
from tools import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ["orbx_frame_create", "orbx_frame_create_from_extraction", "orbx_frame_size", "orbx_frame_read", "orbx_frame_destroy",
               "orbx_frame_search_by_projection_last_frame", "orbx_frame_search_by_projection_map_points",
               "orbx_frame_search_by_projection_keyframe"]


def _small_frame(n=8):
    return dict(x=np.linspace(10, 300, n).astype(f32), y=np.linspace(10, 200, n).astype(f32), octave=np.zeros(n, np.int32),
                angle=np.zeros(n, f32), u_right=np.full(n, -1, f32), desc=np.zeros((n, 32), np.uint8), bounds=(0.0, 0.0, 320.0, 240.0))


def _no_gpu(pkg):
    return pkg.lib().orbx_device_count() == 0


# ------------------------------------------------------------------------------------------------ CPU

def test_new_symbols_exported(pkg):
    import __graft_entry__ as ge
    ge.build()
    L = C.CDLL(pkg.lib_path())
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr, n
        assert hasattr(L, n), n
    assert hasattr(pkg, "DeviceFrame")
    for m in ("SearchByProjectionLastFrameResident", "SearchByProjectionMapPointsResident", "SearchByProjectionKeyFrameResident"):
        assert callable(getattr(pkg.ORBmatcher, m)), m


def test_malformed_arguments_rejected(pkg):
    L = pkg.lib()
    h = C.c_void_p()
    ff = pkg.orbx.FrameFeats()

    def expect_invalid(rc):
        assert rc == -1, rc
        assert len(L.orbx_last_error()) > 0

    expect_invalid(L.orbx_frame_create(0, None, C.byref(h)))
    ff.n = -1
    expect_invalid(L.orbx_frame_create(0, C.byref(ff), C.byref(h)))
    ff.n = 70000
    expect_invalid(L.orbx_frame_create(0, C.byref(ff), C.byref(h)))
    ff.n = 4                                                  # arrays missing
    ff.min_x, ff.min_y, ff.max_x, ff.max_y = 0.0, 0.0, 320.0, 240.0
    expect_invalid(L.orbx_frame_create(0, C.byref(ff), C.byref(h)))
    s_, keep = pkg.ORBmatcher._frame(dict(_small_frame(), occupied=None))
    s_.max_x = s_.min_x                                       # empty bounds
    expect_invalid(L.orbx_frame_create(0, C.byref(s_), C.byref(h)))
    expect_invalid(L.orbx_frame_create(0, C.byref(pkg.ORBmatcher._frame(dict(_small_frame(), occupied=None))[0]), None))
    fake = C.c_void_p(4096)
    K = (C.c_float * 4)(500.0, 500.0, 320.0, 240.0); d3 = (C.c_float * 5)(0.1, 0.0, 0.0, 0.0, 0.0)
    ext = L.orbx_frame_create_from_extraction
    expect_invalid(ext(0, None, fake, fake, 100, 0, None, None, None, 0, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)))
    expect_invalid(ext(0, fake, None, fake, 100, 0, None, None, None, 0, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)))
    expect_invalid(ext(0, fake, fake, None, 100, 0, None, None, None, 0, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)))
    expect_invalid(ext(0, fake, fake, fake, 0, 0, None, None, None, 0, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)))      # cap < 1
    expect_invalid(ext(0, fake, fake, fake, 100, -1, None, None, None, 0, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)))   # index < 0
    expect_invalid(ext(0, fake, fake, fake, 100, 0, None, K, None, 0, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)))       # K, no coefficients
    expect_invalid(ext(0, fake, fake, fake, 100, 0, None, K, d3, 3, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)))         # 3 coefficients
    expect_invalid(ext(0, fake, fake, fake, 100, 0, None, None, None, 0, 0.0, 0.0, 0.0, 240.0, None, C.byref(h)))      # empty bounds
    expect_invalid(ext(0, fake, fake, fake, 100, 0, None, None, None, 0, 0.0, 0.0, 320.0, 240.0, None, None))
    assert L.orbx_frame_size(None) == -1
    expect_invalid(L.orbx_frame_read(None, None, None, None, None, None, None))
    L.orbx_frame_destroy(None)
    pts = pkg.orbx.ProjPoints(); sf = (C.c_float * 2)(1.0, 1.2); m = (C.c_int32 * 8)(); n = C.c_int()
    expect_invalid(L.orbx_frame_search_by_projection_last_frame(None, None, C.byref(pts), sf, 2, 7.0, 0, 0.0, 1, m, C.byref(n)))
    expect_invalid(L.orbx_frame_search_by_projection_last_frame(fake, None, C.byref(pts), sf, 2, 7.0, 5, 0.0, 1, m, C.byref(n)))  # direction
    expect_invalid(L.orbx_frame_search_by_projection_map_points(None, None, C.byref(pts), sf, 2, 3.0, 0.8, m, C.byref(n)))
    expect_invalid(L.orbx_frame_search_by_projection_keyframe(None, None, C.byref(pts), sf, 2, 10.0, 100, 1, m, C.byref(n)))
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.DeviceFrame(dict(_small_frame(), bounds=(0.0, 0.0, 0.0, 0.0)))
    assert ei.value.code == -1
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.DeviceFrame.from_extraction(0, 4096, 4096, 4096, 100, -1, bounds=(0.0, 0.0, 320.0, 240.0))
    assert ei.value.code == -1


def test_no_device_no_fallback(pkg):
    """valid arguments on a box without a GPU: ORBX_E_NO_DEVICE, never a host computation"""
    if not _no_gpu(pkg):
        pytest.skip("a GPU is present")
    L = pkg.lib()
    h = C.c_void_p()
    s_, keep = pkg.ORBmatcher._frame(dict(_small_frame(), occupied=None))
    assert L.orbx_frame_create(0, C.byref(s_), C.byref(h)) == -4
    fake = C.c_void_p(4096)
    assert L.orbx_frame_create_from_extraction(0, fake, fake, fake, 100, 0, None, None, None, 0, 0.0, 0.0, 320.0, 240.0, None, C.byref(h)) == -4
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.DeviceFrame(_small_frame())
    assert ei.value.code == -4
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.DeviceFrame.from_extraction(0, 4096, 4096, 4096, 100, 0, bounds=(0.0, 0.0, 320.0, 240.0))
    assert ei.value.code == -4


def test_frame_driver_compiles(tmp_path):
    """the adaptor-cache driver builds against the stub with the adaptor sources tests/test_adapter.py links"""
    _build_frame_driver(str(tmp_path))


# ------------------------------------------------------------------------------------------------ GPU

ADAPTER = [os.path.join(ROOT, "adapter", f) for f in ("ORBextractor.cc", "Frame_stereo.cc", "ORBmatcher_bow.cc", "ORBmatcher_proj.cc", "ORBmatcher_fuse.cc",
                                                       "Frame_bow.cc", "MapPoint_distinctive.cc", "ORBmatcher_batch.cc")]


def _build_frame_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_frame_driver")
    inc = ["-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-DORBX_ADAPTER_CAPTURE"] + inc +
                          [os.path.join(ROOT, "tests", "adapter_frame_driver.cc")] + ADAPTER +
                          ["-L", os.path.join(ROOT, "orb-slam2_amd"), "-lorbx", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "orb-slam2_amd"), "-o", exe])
    return exe


def _frame_only(cur):
    return {k: cur[k] for k in ("x", "y", "octave", "angle", "u_right", "desc", "bounds")}


def _check_all(pkg, oracle, df, cur, pts, sf, tag):
    """every resident search of one frame == host-pointer twin == oracle"""
    occ = cur["occupied"]
    for co in (0, 1, 3):
        mt = pkg.ORBmatcher(0.9, co != 0)
        for direction, th in ((0, 15.0), (1, 7.0), (2, 7.0)):
            got, n = mt.SearchByProjectionLastFrameResident(df, occ, pts, sf, th, direction, 40.0, check_orientation=co)
            if co == 3:   # the host-pointer wrapper passes mbCheckOrientation as 0 / 1: call the ABI with 3 directly
                a, ka = pkg.ORBmatcher._frame(cur); b, kb = pkg.ORBmatcher._points(pts)
                hg = np.full(a.n, -1, np.int32); hn = C.c_int()
                rc = pkg.lib().orbx_search_by_projection_last_frame(0, C.byref(a), C.byref(b), sf.ctypes.data, len(sf), th, direction, 40.0, 3,
                                                                    hg.ctypes.data, C.byref(hn))
                assert rc == 0
                hn = hn.value
            else:
                hg, hn = mt.SearchByProjectionLastFrame(cur, pts, sf, th, direction, 40.0)
            exp, en = oracle.search_by_projection_last(cur, pts, sf, th, direction, 40.0, co)
            assert n == hn == en, (tag, "last", co, direction, n, hn, en)
            assert (got == hg).all() and (got == exp).all(), (tag, "last", co, direction, np.nonzero(got != exp)[0][:5])
    p2 = dict(pts); p2["aux"] = (pts["u"] - 5).astype(f32)
    for th, ratio in ((1.0, 0.8), (3.0, 0.8), (5.0, 0.6)):
        mt = pkg.ORBmatcher(ratio, True)
        got, n = mt.SearchByProjectionMapPointsResident(df, occ, p2, sf, th)
        hg, hn = mt.SearchByProjectionMapPoints(cur, p2, sf, th)
        exp, en = oracle.search_by_projection_points(cur, p2, sf, th, ratio)
        assert n == hn == en and (got == hg).all() and (got == exp).all(), (tag, "points", th)
    for ori in (False, True):
        mt = pkg.ORBmatcher(0.9, ori)
        for th, od in ((10.0, 100), (3.0, 64)):
            got, n = mt.SearchByProjectionKeyFrameResident(df, occ, pts, sf, th, od)
            hg, hn = mt.SearchByProjectionKeyFrame(cur, pts, sf, th, od)
            exp, en = oracle.search_by_projection_keyframe(cur, pts, sf, th, od, ori)
            assert n == hn == en and (got == hg).all() and (got == exp).all(), (tag, "kf", ori, th)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,dense,obs", [(3, False, 0.7), (4, True, 0.7), (5, True, 1.0), (6, True, 0.0), (7, False, 0.3)])
def test_resident_parity_one_frame(pkg, oracle, seed, dense, obs):
    cur, pts, sf = _scene(seed, 1200, 1000, dense=dense, obs_frac=obs)
    df = pkg.DeviceFrame(_frame_only(cur))
    assert df.n == len(cur["x"])
    _check_all(pkg, oracle, df, cur, pts, sf, seed)
    back = df.read()
    for k in ("x", "y", "octave", "angle", "u_right", "desc"):
        assert back[k].tobytes() == np.ascontiguousarray(cur[k]).tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("seed,dense", [(3, False), (4, True)])
def test_occupied_changes_between_calls(pkg, oracle, seed, dense):
    """TrackWithMotionModel at th with occupied as given, again at 2*th with everything cleared, then SearchLocalPoints with occupied
    derived from the previous result -- one frame, three calls"""
    cur, pts, sf = _scene(seed, 1000, 1000, dense=dense)
    df = pkg.DeviceFrame(_frame_only(cur))
    mt = pkg.ORBmatcher(0.9, True)
    th = 7.0
    got, n = mt.SearchByProjectionLastFrameResident(df, cur["occupied"], pts, sf, th, 0, 40.0)
    exp, en = oracle.search_by_projection_last(cur, pts, sf, th, 0, 40.0, True)
    assert n == en and (got == exp).all()
    clear = np.zeros(df.n, np.uint8)
    got2, n2 = mt.SearchByProjectionLastFrameResident(df, clear, pts, sf, 2 * th, 0, 40.0)
    c2 = dict(cur, occupied=clear)
    exp2, en2 = oracle.search_by_projection_last(c2, pts, sf, 2 * th, 0, 40.0, True)
    assert n2 == en2 and (got2 == exp2).all() and n2 > 20
    gn, gnn = mt.SearchByProjectionLastFrameResident(df, None, pts, sf, 2 * th, 0, 40.0)
    assert gnn == n2 and (gn == got2).all()                      # None == all zeros
    occ3 = ((got2 >= 0) & (pts["has_obs"][np.maximum(got2, 0)] == 1)).astype(np.uint8)   # features now holding an observed point
    p2 = dict(pts); p2["aux"] = (pts["u"] - 5).astype(f32)
    ml = pkg.ORBmatcher(0.8, True)
    got3, n3 = ml.SearchByProjectionMapPointsResident(df, occ3, p2, sf, 3.0)
    exp3, en3 = oracle.search_by_projection_points(dict(cur, occupied=occ3), p2, sf, 3.0, 0.8)
    assert n3 == en3 and (got3 == exp3).all() and n3 > 20
    with pytest.raises(pkg.OrbxError):
        ml.SearchByProjectionMapPointsResident(df, occ3[:-1], p2, sf, 3.0)


def _points_for(frame, seed, n_pts=900):
    """points projected near the frame's features (as a last frame's points would be), descriptors a few bits away"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nf = len(frame["x"])
    src = rng.integers(0, nf, n_pts)
    return dict(u=(frame["x"][src] + rng.normal(0, 3, n_pts)).astype(f32), v=(frame["y"][src] + rng.normal(0, 3, n_pts)).astype(f32),
                aux=rng.uniform(0.02, 0.5, n_pts).astype(f32), level=frame["octave"][src].astype(np.int32),
                angle=((frame["angle"][src] + rng.normal(0, 8, n_pts)) % 360).astype(f32), view_cos=rng.uniform(0.99, 1.0, n_pts).astype(f32),
                desc=synth.flip_bits(rng, frame["desc"][src], 0.06), valid=(rng.random(n_pts) < 0.92).astype(np.uint8),
                has_obs=(rng.random(n_pts) < 0.7).astype(np.uint8))


W, H = 1241, 376
BF, MIN_Z = 386.1448, 386.1448 / 718.856


def _extract_pair(pkg, ex, imgs, kps, desc, nout, ur, dp, pairs, pitch, sp):
    import torch
    host = np.zeros((2, H, pitch), np.uint8)
    host[0, :, :W] = pairs[0]; host[1, :, :W] = pairs[1]
    imgs.copy_(torch.from_numpy(host))
    cap = kps.shape[1]
    ex.extract_batch_device(imgs.data_ptr(), H * pitch, pitch, 2, W, H, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), sp)
    pkg.orbx.stereo_match_batch_device(ex, 0, ex, 1, 1, kps.data_ptr(), desc.data_ptr(), nout.data_ptr(), kps[1:].data_ptr(), desc[1:].data_ptr(),
                                       nout[1:].data_ptr(), cap, BF, MIN_Z, ur.data_ptr(), dp.data_ptr(), sp)


@pytest.mark.gpu
def test_from_extraction_buffers(pkg, oracle):
    import torch
    dev = torch.device("cuda", 0)
    pitch = (W + 63) // 64 * 64
    ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=2)
    cap = ex.max_keypoints(W, H)
    imgs = torch.zeros((2, H, pitch), dtype=torch.uint8, device=dev)
    kps = torch.zeros((2, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros(2, dtype=torch.int32, device=dev)
    ur = torch.full((1, cap), 123.0, dtype=torch.float32, device=dev)
    dp = torch.zeros((1, cap), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    l0, r0, _ = synth.stereo_pair(901, W, H)
    _extract_pair(pkg, ex, imgs, kps, desc, nout, ur, dp, (l0, r0), pitch, sp)
    bounds = (0.0, 0.0, float(W), float(H))
    st = pkg.DeviceFrame.from_extraction(0, kps.data_ptr(), desc.data_ptr(), nout.data_ptr(), cap, 0, d_u_right=ur.data_ptr(), bounds=bounds, stream=sp)
    mono = pkg.DeviceFrame.from_extraction(0, kps.data_ptr(), desc.data_ptr(), nout.data_ptr(), cap, 0, bounds=bounds, stream=sp)
    ex.sync(sp)
    n = int(nout[0].item())
    k_host = kps[0, :n].cpu().numpy().copy().view(pkg.KP_DTYPE).reshape(n)
    d_host = desc[0, :n].cpu().numpy().copy()
    u_host = ur[0, :n].cpu().numpy().copy()
    assert st.n == n == mono.n and n > 500 and (u_host >= 0).sum() > 100
    fs, fm = st.read(), mono.read()
    for f_ in (fs, fm):
        assert f_["x"].tobytes() == k_host["x"].tobytes() and f_["y"].tobytes() == k_host["y"].tobytes()
        assert f_["octave"].tobytes() == k_host["octave"].tobytes() and f_["angle"].tobytes() == k_host["angle"].tobytes()
        assert f_["desc"].tobytes() == d_host.tobytes()
    assert fs["u_right"].tobytes() == u_host.tobytes() and (fm["u_right"] == -1).all()
    sf = ex.GetScaleFactors()
    results = {}
    for name, df, rb in (("stereo", st, fs), ("mono", mono, fm)):
        cur = dict(rb, occupied=np.zeros(n, np.uint8), bounds=bounds)
        pts = _points_for(cur, 77)
        mt = pkg.ORBmatcher(0.9, True)
        got, gn = mt.SearchByProjectionLastFrameResident(df, None, pts, sf, 7.0, 0, BF)
        hg, hn = mt.SearchByProjectionLastFrame(cur, pts, sf, 7.0, 0, BF)
        assert gn == hn and (got == hg).all() and gn > 100, name
        p2 = dict(pts); p2["aux"] = (pts["u"] - 5).astype(f32)
        got2, gn2 = mt.SearchByProjectionMapPointsResident(df, None, p2, sf, 3.0)
        hg2, hn2 = mt.SearchByProjectionMapPoints(cur, p2, sf, 3.0)
        assert gn2 == hn2 and (got2 == hg2).all(), name
        results[name] = (pts, p2, got, gn, got2, gn2)
    # the frames own their data: a second extraction of other images into the same buffers changes nothing
    l1, r1, _ = synth.stereo_pair(902, W, H)
    _extract_pair(pkg, ex, imgs, kps, desc, nout, ur, dp, (l1, r1), pitch, sp)
    ex.sync(sp)
    assert kps[0, :50].cpu().numpy().tobytes() != k_host[:50].tobytes()
    for name, df in (("stereo", st), ("mono", mono)):
        pts, p2, got, gn, got2, gn2 = results[name]
        mt = pkg.ORBmatcher(0.9, True)
        a, an = mt.SearchByProjectionLastFrameResident(df, None, pts, sf, 7.0, 0, BF)
        b, bn = mt.SearchByProjectionMapPointsResident(df, None, p2, sf, 3.0)
        assert an == gn and (a == got).all() and bn == gn2 and (b == got2).all(), name
    assert st.read()["x"].tobytes() == fs["x"].tobytes()


def _fake_extraction(kp_dtype, seed, n, cap, batch=2, w=W, h=H):
    """extraction-shaped device buffers written from the host (keypoint records, descriptors, counts): image 1 holds the frame"""
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.zeros((batch, cap), kp_dtype)
    k["x"][1, :n] = rng.uniform(0, w, n); k["y"][1, :n] = rng.uniform(0, h, n); k["angle"][1, :n] = rng.uniform(0, 360, n)
    k["octave"][1, :n] = rng.integers(0, 8, n); k["size"][1, :n] = 31; k["response"][1, :n] = rng.uniform(0, 100, n)
    d = rng.integers(0, 256, (batch, cap, 32), dtype=np.uint8)
    u = np.full((batch, cap), 55.5, np.float32); u[1, :n] = np.where(rng.random(n) < 0.5, k["x"][1, :n] - rng.uniform(1, 30, n), -1)
    cnt = np.array([cap // 3, n] + [0] * (batch - 2), np.int32)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev) for a in (k, d, u, cnt)]
    torch.cuda.synchronize()
    return t, k[1, :n], d[1, :n], u[1, :n]


@pytest.mark.gpu
def test_undistortion_on_device(pkg):
    n, cap = 1500, 2000
    (tk, td, tu, tn), k, d, u = _fake_extraction(pkg.KP_DTYPE, 41, n, cap)
    Kc = (517.3, 516.5, 318.6, 255.3)
    dist = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633], np.float32)
    b = (0.0, 0.0, float(W), float(H))
    f = pkg.DeviceFrame.from_extraction(0, tk.data_ptr(), td.data_ptr(), tn.data_ptr(), cap, 1, d_u_right=tu.data_ptr() + 4 * cap, K=Kc, dist_coef=dist, bounds=b)
    r = f.read()
    exp = pkg.UndistortKeyPoints(np.stack([k["x"], k["y"]], 1), *Kc, dist)
    assert r["x"].tobytes() == np.ascontiguousarray(exp[:, 0]).tobytes() and r["y"].tobytes() == np.ascontiguousarray(exp[:, 1]).tobytes()
    assert not np.array_equal(r["x"], k["x"])
    assert r["octave"].tobytes() == k["octave"].tobytes() and r["angle"].tobytes() == k["angle"].tobytes()
    assert r["desc"].tobytes() == d.tobytes() and r["u_right"].tobytes() == u.tobytes()
    d0 = dist.copy(); d0[0] = 0.0
    g = pkg.DeviceFrame.from_extraction(0, tk.data_ptr(), td.data_ptr(), tn.data_ptr(), cap, 1, K=Kc, dist_coef=d0, bounds=b).read()
    assert g["x"].tobytes() == k["x"].tobytes() and g["y"].tobytes() == k["y"].tobytes() and (g["u_right"] == -1).all()


@pytest.mark.gpu
def test_edges(pkg, oracle):
    mt = pkg.ORBmatcher(0.9, True)
    cur, pts, sf = _scene(9, 300, 200)
    # an n = 0 frame
    empty = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in _frame_only(cur).items()}
    e = pkg.DeviceFrame(empty)
    assert e.n == 0 and e.read()["x"].size == 0
    got, n = mt.SearchByProjectionLastFrameResident(e, None, pts, sf, 7.0)
    assert n == 0 and got.size == 0
    # more than 8192 features: the grid in global memory -- from host pointers and from extraction-shaped buffers
    big, bpts, bsf = _scene(10, 10000, 3000, w=1241, h=376)
    bf = pkg.DeviceFrame(_frame_only(big))
    got, n = mt.SearchByProjectionLastFrameResident(bf, big["occupied"], bpts, bsf, 7.0, 0, 40.0)
    exp, en = oracle.search_by_projection_last(big, bpts, bsf, 7.0, 0, 40.0, True)
    assert n == en and (got == exp).all() and n > 100
    nb, cap = 9000, 9500
    (tk, td, tu, tn), k, d, u = _fake_extraction(pkg.KP_DTYPE, 43, nb, cap)
    fe = pkg.DeviceFrame.from_extraction(0, tk.data_ptr(), td.data_ptr(), tn.data_ptr(), cap, 1, d_u_right=tu.data_ptr() + 4 * cap,
                                         bounds=(0.0, 0.0, float(W), float(H)))
    r = fe.read()
    assert fe.n == nb and r["x"].tobytes() == k["x"].tobytes() and r["u_right"].tobytes() == u.tobytes() and r["desc"].tobytes() == d.tobytes()
    fcur = dict(r, occupied=np.zeros(nb, np.uint8), bounds=(0.0, 0.0, float(W), float(H)))
    fpts = _points_for(fcur, 5, 2500)
    got, n = mt.SearchByProjectionLastFrameResident(fe, None, fpts, bsf, 7.0, 0, 40.0)
    exp, en = oracle.search_by_projection_last(fcur, fpts, bsf, 7.0, 0, 40.0, True)
    assert n == en and (got == exp).all() and n > 100
    # a point level >= nlevels
    bad = dict(bpts); bad["level"] = bpts["level"].copy(); bad["level"][0] = 12; bad["valid"] = bpts["valid"].copy(); bad["valid"][0] = 1
    with pytest.raises(pkg.OrbxError):
        mt.SearchByProjectionLastFrameResident(bf, None, bad, bsf, 7.0)
    # index / cap misuse: image 0 claims cap // 3 keypoints, a cap below that is refused, as are a negative index and a zero cap
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.DeviceFrame.from_extraction(0, tk.data_ptr(), td.data_ptr(), tn.data_ptr(), 100, 1, bounds=(0.0, 0.0, float(W), float(H)))
    assert ei.value.code == -1
    for cap_, idx in ((cap, -1), (0, 0)):
        with pytest.raises(pkg.OrbxError):
            pkg.DeviceFrame.from_extraction(0, tk.data_ptr(), td.data_ptr(), tn.data_ptr(), cap_, idx, bounds=(0.0, 0.0, float(W), float(H)))


@pytest.mark.gpu
def test_adaptor_resident_frame_cache(tmp_path):
    exe = _build_frame_driver(str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    vals = dict(line.split(" ", 1) for line in run.stdout.strip().splitlines() if " " in line)
    assert vals["equal_direct"] == "1" and vals["creates"] == "1" and vals["hits"] == "3", out
    assert vals["rebuilt"] == "1" and vals["equal_off"] == "1", out
    print(out)
