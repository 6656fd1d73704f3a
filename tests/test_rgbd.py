"""RGB-D frames on the device: Tracking::GrabImageRGBD's image preparation (reference src/Tracking.cc:217-233) and the RGB-D constructor's
ExtractORB / UndistortKeyPoints / ComputeStereoFromRGBD (src/Frame.cc:145-154, :470-515, :754-774) through orbx_extract_rgbd, its pipelined
form, orbx_rgbd_depth_batch_device and the C++ adaptor ORBextractor::ExtractRGBD.

Expected values come from a numpy restatement (np.float32 multiply, division and subtraction; keypoints from the C oracle; undistorted
positions from oracle_py.undistort_points), itself checked against a line-by-line transcription of Frame.cc:754-774.  Constants: the
TUM1-3 RGB-D settings (tests/golden/reference_settings_rgbd.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tools import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_settings_rgbd.json")))
TUM1, TUM3 = FIX["TUM1 rgbd"], FIX["TUM3 rgbd"]          # TUM3: no distortion (k1 = 0)
W, H = int(TUM1["Camera.width"]), int(TUM1["Camera.height"])
NF = int(TUM1["ORBextractor.nFeatures"])
f32 = np.float32
NEW_SYMBOLS = ["orbx_extract_rgbd", "orbx_extract_rgbd_submit", "orbx_extract_rgbd_wait", "orbx_rgbd_depth_batch_device"]


# ------------------------------------------------------------------------------------------------ the expected values

def transcription(kx, ky, kux, imDepth, mbf):
    """Frame::ComputeStereoFromRGBD (src/Frame.cc:754-774) line by line over np.float32 scalars; imDepth = the CV_32F matrix Tracking made"""
    N = len(kx)
    mvuRight = [f32(-1)] * N
    mvDepth = [f32(-1)] * N
    for i in range(N):
        v = f32(ky[i])
        u = f32(kx[i])
        d = f32(imDepth[int(v), int(u)])     # at<float>(v, u): the implicit float -> int conversion truncates
        if d > 0:
            mvDepth[i] = d
            with np.errstate(over="ignore"):     # a denormal d: mbf / d overflows to inf, as in fp32 C++
                mvuRight[i] = f32(f32(kux[i]) - f32(mbf) / d)
    return np.array(mvuRight, f32), np.array(mvDepth, f32)


def convert_depth(raw, depth_scale):
    """src/Tracking.cc:232-233: if((fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F) imDepth.convertTo(imDepth,CV_32F,mDepthMapFactor)"""
    s = f32(depth_scale)
    if raw.dtype != np.float32 or float(np.abs(s - f32(1))) > 1e-5:
        return raw.astype(f32) * s
    return raw.astype(f32)


def restate(kx, ky, kux, raw, depth_scale, bf):
    """vectorised restatement: (u_right, depth); a truncated position outside the image (the library's defined deviation) gives -1 / -1"""
    kx = np.asarray(kx, f32); ky = np.asarray(ky, f32); kux = np.asarray(kux, f32)
    d_img = convert_depth(raw, depth_scale)
    h, w = d_img.shape
    with np.errstate(invalid="ignore"):
        ok = (kx > -1) & (kx < w) & (ky > -1) & (ky < h)
    u = np.where(ok, np.trunc(np.where(ok, kx, 0)), 0).astype(np.int64)
    v = np.where(ok, np.trunc(np.where(ok, ky, 0)), 0).astype(np.int64)
    d = np.where(ok, d_img[v, u], f32(-1)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pos = d > 0
        ur = np.where(pos, kux - f32(bf) / np.where(pos, d, f32(1)), f32(-1)).astype(f32)
    return ur, np.where(pos, d, f32(-1)).astype(f32)


def params(pkg, cam, dist=True, **kw):
    d = [cam["Camera.k1"], cam["Camera.k2"], cam["Camera.p1"], cam["Camera.p2"]] + ([cam["Camera.k3"]] if "Camera.k3" in cam else [])
    if not dist:
        d = [0.0] * len(d)
    return pkg.RGBDParams(cam["Camera.fx"], cam["Camera.fy"], cam["Camera.cx"], cam["Camera.cy"], d, cam["Camera.bf"],
                          **(kw or dict(DepthMapFactor=cam["DepthMapFactor"])))


def _u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _colour(seed, ch):
    return np.stack([synth.image(seed + 17 * c, W, H) for c in range(ch)], 2)


def _gray_of(img, rgb):
    """cvtColor(CV_RGB2GRAY / CV_BGR2GRAY ...) for 8U: fixed point, yuv_shift 14 (the arithmetic of k_gray)"""
    c = img.astype(np.int64)
    r, g, b = (c[..., 0], c[..., 1], c[..., 2]) if rgb else (c[..., 2], c[..., 1], c[..., 0])
    return ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def _depth_u16(seed, w=W, h=H):
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.integers(2500, 30000, (h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.08] = 0                       # holes
    d[rng.random((h, w)) < 0.01] = 65535
    return d


def _depth_f32(seed, w=W, h=H):
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.uniform(0.3, 6.0, (h, w)).astype(f32)
    m = rng.random((h, w))
    d[m < 0.05] = 0; d[(m >= 0.05) & (m < 0.07)] = -1.5; d[(m >= 0.07) & (m < 0.08)] = np.nan
    return d


def _oracle_undistort(oracle, kps, cam, dist=True):
    xy = np.stack([kps["x"], kps["y"]], 1).astype(f32)
    if not dist or cam["Camera.k1"] == 0:
        return xy
    d = [cam["Camera.k1"], cam["Camera.k2"], cam["Camera.p1"], cam["Camera.p2"]] + ([cam["Camera.k3"]] if "Camera.k3" in cam else [])
    return oracle.undistort_points(xy, cam["Camera.fx"], cam["Camera.fy"], cam["Camera.cx"], cam["Camera.cy"], d)


# ------------------------------------------------------------------------------------------------ CPU

def test_new_symbols_exported(pkg):
    import __graft_entry__ as ge
    ge.build()
    L = C.CDLL(pkg.lib_path())
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr, n
        assert hasattr(L, n), n
    assert "ORBX_DEPTH_U16" in hdr and "ORBX_DEPTH_F32" in hdr and "orbx_rgbd_params" in hdr
    for m in ("extract_rgbd", "extract_rgbd_submit", "extract_rgbd_wait"):
        assert callable(getattr(pkg.ORBextractor, m)), m
    assert callable(pkg.rgbd_depth_batch_device) and callable(pkg.depth_map_factor) and pkg.RGBDParams


def test_depth_map_factor(pkg):
    """src/Tracking.cc:147-151 in float32"""
    assert pkg.depth_map_factor(5000).tobytes() == (f32(1) / f32(5000)).tobytes()
    assert pkg.depth_map_factor(5208.0).tobytes() == (f32(1) / f32(5208)).tobytes()
    assert pkg.depth_map_factor(1e-6) == f32(1) and pkg.depth_map_factor(0) == f32(1) and pkg.depth_map_factor(1) == f32(1)
    p = pkg.RGBDParams.from_settings(TUM1)
    assert p.depth_scale == f32(1) / f32(5000) and p.bf == f32(40) and len(p.dist_coef) == 5


def test_fixture_matches_reference_settings():
    """the RGB-D fixture as tools/gen_settings_fixture.py writes it; re-derived from the yaml files where the reference checkout is present"""
    from tools import gen_settings_fixture as g
    assert sorted(FIX) == sorted(g.RGBD_FILES)
    for name, rel in g.RGBD_FILES.items():
        assert FIX[name]["file"] == "Examples/" + rel
        assert set(g.RGBD_KEYS) - {"Camera.k3"} <= set(FIX[name]) - {"file"} <= set(g.RGBD_KEYS), name   # TUM3.yaml has four coefficients
        path = os.path.join(g.REF, rel)
        if os.path.exists(path):
            assert g.parse(path, g.RGBD_KEYS) == {k: v for k, v in FIX[name].items() if k != "file"}, name
    assert (TUM1["Camera.k1"], TUM1["Camera.k2"], TUM1["Camera.k3"]) == (0.262383, -0.953104, 1.163314)
    assert TUM1["DepthMapFactor"] == 5000.0 and TUM1["Camera.bf"] == 40.0 and (W, H) == (640, 480)


def test_restatement_matches_transcription():
    """the numpy restatement == the line-by-line transcription of Frame.cc:754-774, edge values included"""
    rng = np.random.Generator(np.random.PCG64(5))
    w, h = 64, 48
    vals_f = np.array([0, -0.0, -1, np.nan, np.inf, -np.inf, np.finfo(f32).smallest_subnormal, 1e30, 2.5, 1e-30, 3.75e-39], f32)
    vals_u = np.array([0, 1, 2, 1000, 5000, 65534, 65535], np.uint16)
    n = 3000
    kx = np.concatenate([rng.integers(0, w, 200).astype(f32), rng.integers(0, w, 200) + f32(0.999), rng.uniform(0, w - 1e-3, n)]).astype(f32)
    ky = np.concatenate([rng.integers(0, h, 200).astype(f32), rng.integers(0, h, 200) + f32(0.999), rng.uniform(0, h - 1e-3, n)]).astype(f32)
    kux = (kx + rng.normal(0, 3, len(kx))).astype(f32)
    for raw in (vals_f[rng.integers(0, len(vals_f), (h, w))], rng.uniform(-2, 8, (h, w)).astype(f32),
                vals_u[rng.integers(0, len(vals_u), (h, w))], rng.integers(0, 65536, (h, w)).astype(np.uint16)):
        for scale in (f32(1), f32(1.000005), f32(1.00002), f32(1) / f32(5000), f32(1) / f32(5208)):
            for bf in (40.0, 386.1448):
                ur, z = restate(kx, ky, kux, raw, scale, bf)
                tu, tz = transcription(kx, ky, kux, convert_depth(raw, scale), bf)
                assert (_u32(ur) == _u32(tu)).all() and (_u32(z) == _u32(tz)).all(), (raw.dtype, scale, bf)
    # the consequences the library keeps
    one = np.ones((1, 8), f32)
    for v, exp_ur in ((np.nan, -1), (np.inf, 10.0), (np.finfo(f32).smallest_subnormal, -np.inf), (0, -1), (-3, -1)):
        ur, z = restate([1.5], [0.5], [10.0], one * f32(v), 1.0, 40.0)
        assert ur[0] == exp_ur or (np.isnan(exp_ur) and np.isnan(ur[0])), (v, ur)
    # the scale rule: 1.000005 is not applied to float depth, 1.00002 is; uint16 depth is always converted
    assert convert_depth(one * f32(3), f32(1.000005))[0, 0] == f32(3)
    assert convert_depth(one * f32(3), f32(1.00002))[0, 0] == f32(3) * f32(1.00002)
    assert convert_depth(np.full((1, 2), 3, np.uint16), f32(1))[0, 0] == f32(3)


def test_refusals_without_device(pkg):
    """argument checks come first (ORBX_E_INVALID), then the device (ORBX_E_NO_DEVICE: there is no CPU fallback)"""
    L = pkg.lib()
    p = params(pkg, TUM1)
    fake = 4096

    def batch(pp=None, cap=1000, batch_=1, img_stride=0, pitch=1280, w=W, h=H, kps=fake, n=fake, dep=fake, ur=fake, z=fake, dt=pkg.DEPTH_U16):
        s = (pp or p).struct(dt)
        return L.orbx_rgbd_depth_batch_device(0, kps, n, cap, batch_, dep, img_stride, pitch, w, h, C.byref(s), None, ur, z, None)

    assert batch(kps=None) == -1 and batch(n=None) == -1 and batch(dep=None) == -1 and batch(ur=None) == -1 and batch(z=None) == -1
    assert batch(cap=0) == -1 and batch(batch_=0) == -1 and batch(w=0) == -1 and batch(h=0) == -1
    assert batch(dt=7) == -1                                    # unknown depth_type
    assert batch(pitch=1279) == -1 and batch(pitch=1281) == -1  # below a row / not a multiple of the element size (u16)
    assert batch(pitch=2558, dt=pkg.DEPTH_F32) == -1 and batch(pitch=2562, dt=pkg.DEPTH_F32) == -1
    assert batch(batch_=2, img_stride=1280 * H - 2) == -1       # images overlap
    p3 = params(pkg, TUM1); p3.dist_coef = p3.dist_coef[:3]
    assert batch(pp=p3) == -1                                   # ndist not 4 or 5
    assert L.orbx_rgbd_depth_batch_device(0, fake, fake, 1000, 1, fake, 0, 1280, W, H, None, None, fake, fake, None) == -1
    s = p.struct(pkg.DEPTH_U16)
    buf = np.zeros(16, np.uint8)
    n = C.c_int()
    assert L.orbx_extract_rgbd(None, buf.ctypes.data, W, H, W, 1, 1, buf.ctypes.data, 1280, C.byref(s), buf.ctypes.data, buf.ctypes.data, 10,
                               C.byref(n), None, buf.ctypes.data, buf.ctypes.data) == -1
    t = C.c_int()
    assert L.orbx_extract_rgbd_submit(None, buf.ctypes.data, W, H, W, 1, 1, buf.ctypes.data, 1280, C.byref(s), C.byref(t)) == -1
    assert L.orbx_extract_rgbd_wait(None, 0, buf.ctypes.data, buf.ctypes.data, 10, C.byref(n), None, buf.ctypes.data, buf.ctypes.data) == -1
    if L.orbx_device_count() == 0:
        assert batch() == -4
        assert "no CPU fallback" in L.orbx_last_error().decode()
        with pytest.raises(pkg.OrbxError):
            pkg.ORBextractor(NF, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=2)


def _compile_flags():
    return ["-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_rgbd"), "-I", os.path.join(ROOT, "tests", "cvstub"),
            "-I", os.path.join(ROOT, "include")]


def test_adaptor_compiles():
    """adapter/ORBextractor_rgbd.cc against the stub (+ tests/cvstub_rgbd for CV_16U), warnings as errors"""
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + _compile_flags() +
                          [os.path.join(ROOT, "adapter", "ORBextractor_rgbd.cc")])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + _compile_flags() +
                          [os.path.join(ROOT, "tests", "adapter_rgbd_driver.cc")])


# ------------------------------------------------------------------------------------------------ GPU

def _ex(pkg, max_batch=2):
    return pkg.ORBextractor(NF, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=max_batch)


def _check_frame(tag, got, exp):
    k, d, xy, ur, z = got
    ek, ed, exy, eur, ez = exp
    assert len(k) == len(ek) and k.tobytes() == ek.tobytes() and d.tobytes() == ed.tobytes(), f"{tag}: keypoints / descriptors"
    assert xy.tobytes() == np.ascontiguousarray(exy, f32).tobytes(), f"{tag}: undistorted positions"
    bad = np.nonzero(_u32(ur) != _u32(eur))[0]
    assert len(bad) == 0, f"{tag}: u_right differs at {bad[:5].tolist()}: {ur[bad[:5]]} vs {eur[bad[:5]]}"
    assert (_u32(z) == _u32(ez)).all(), f"{tag}: depth"


def _expected(pkg, oracle, gray, raw, cam, dist, scale=None):
    kps, desc = oracle.Oracle(NF, 1.2, 8, 20, 7).extract(gray)
    xy = _oracle_undistort(oracle, kps, cam, dist)
    s = f32(1) / f32(cam["DepthMapFactor"]) if scale is None else scale
    ur, z = restate(kps["x"], kps["y"], xy[:, 0], raw, s, cam["Camera.bf"])
    return kps, desc, xy, ur, z


@pytest.mark.gpu
@pytest.mark.parametrize("ch,rgb", [(1, 1), (3, 1), (3, 0), (4, 1), (4, 0)])
@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("dist", [True, False])
def test_one_call_parity(pkg, oracle, ch, rgb, dtype, dist):
    """TUM1 at 640 x 480 @ 1000: keypoints / descriptors == orbx_extract(_color) == oracle, xy_un == orbx_undistort_keypoints, u_right /
    depth == the restatement, bit for bit"""
    ex = _ex(pkg)
    seed = 40 + ch * 3 + rgb
    img = synth.image(seed, W, H) if ch == 1 else _colour(seed, ch)
    gray = img if ch == 1 else _gray_of(img, rgb)
    raw = _depth_u16(seed) if dtype == "u16" else _depth_f32(seed)
    p = params(pkg, TUM1, dist)
    got = ex.extract_rgbd(img, raw, p, rgb=bool(rgb))
    exp = _expected(pkg, oracle, gray, raw, TUM1, dist)
    _check_frame(f"ch{ch} rgb{rgb} {dtype} dist{dist}", got, exp)
    k0, d0 = ex(gray) if ch == 1 else ex.extract_color(img, rgb=bool(rgb))
    assert got[0].tobytes() == k0.tobytes() and got[1].tobytes() == d0.tobytes()
    xy = np.stack([got[0]["x"], got[0]["y"]], 1)
    un = pkg.UndistortKeyPoints(xy, TUM1["Camera.fx"], TUM1["Camera.fy"], TUM1["Camera.cx"], TUM1["Camera.cy"], p.dist_coef)
    assert un.tobytes() == got[2].tobytes()
    assert len(got[0]) > 500 and (got[4] > 0).sum() > 300


@pytest.mark.gpu
def test_lookup_uses_distorted_position(pkg, oracle):
    """a depth map whose value encodes its pixel index, strong distortion: the lookup must use kp, u_right kpU.x"""
    ex = _ex(pkg)
    img = synth.image(71, W, H)
    idx = (np.arange(H)[:, None] * W + np.arange(W)[None, :] + 1).astype(f32)     # exact in fp32 (< 2^24)
    cam = dict(TUM1, **{"Camera.k1": 0.55, "Camera.k2": -0.2, "Camera.p1": 0.004, "Camera.p2": -0.003, "Camera.k3": 0.1})
    p = params(pkg, cam, depth_scale=1.0)
    k, d, xy, ur, z = ex.extract_rgbd(img, idx, p)
    ok, _ = oracle.Oracle(NF, 1.2, 8, 20, 7).extract(img)
    assert k.tobytes() == ok.tobytes()
    exy = _oracle_undistort(oracle, ok, cam)
    assert xy.tobytes() == exy.tobytes()
    eur, ez = restate(k["x"], k["y"], xy[:, 0], idx, 1.0, cam["Camera.bf"])
    assert (_u32(ur) == _u32(eur)).all() and (_u32(z) == _u32(ez)).all()
    # the lookup position is visible in the value: kp's pixel, not kpU's
    assert (z == (np.trunc(k["y"]) * W + np.trunc(k["x"]) + 1).astype(f32)).all()
    wrong_z = restate(xy[:, 0], xy[:, 1], xy[:, 0], idx, 1.0, cam["Camera.bf"])[1]
    assert (wrong_z != z).mean() > 0.5
    wrong_ur = restate(k["x"], k["y"], k["x"], idx, 1.0, cam["Camera.bf"])[0]
    assert (wrong_ur != ur).mean() > 0.5


def _device_keypoints(pkg, xs, ys, cap, batch=1, counts=None):
    import torch
    k = np.zeros((batch, cap), pkg.KP_DTYPE)
    n = len(xs)
    k["x"][0, :n] = xs; k["y"][0, :n] = ys
    cnt = np.array(counts if counts is not None else [n] * batch, np.int32)
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(k.view(np.uint8).reshape(-1).copy()).to(dev), torch.from_numpy(cnt).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1.000005, 1.00002])
def test_edge_values(pkg, scale):
    """f32 depth 0, -1, NaN, +inf, the smallest denormal, 1e30 at integer and x.999 positions; scales 1 / 1.000005 (not applied) /
    1.00002 (applied); positions whose truncation falls outside the image get -1 / -1"""
    import torch
    dev = torch.device("cuda", 0)
    w, h = 16, 4
    vals = np.array([0, -1, np.nan, np.inf, np.finfo(f32).smallest_subnormal, 1e30, 2.5, 0.7], f32)
    raw = np.tile(np.repeat(vals, 2), (h, 1)).astype(f32)                # columns 2i, 2i+1 hold vals[i]
    xs, ys = [], []
    for c in range(w):
        for r in range(h):
            xs += [c, c + 0.999, c + 0.5]; ys += [r, r + 0.999, r + 0.25]
    xs += [-0.5, -1.0, -1.5, w - 0.001, w, w + 3, np.nan, 3, 3]; ys += [0.5, 1, 1, 1, 1, 1, 1, -0.5, h]
    xs = np.array(xs, f32); ys = np.array(ys, f32)
    cap = 256
    dk, dn = _device_keypoints(pkg, xs, ys, cap)
    ddep = torch.from_numpy(raw.copy()).to(dev)
    ur = torch.full((cap,), 123.0, dtype=torch.float32, device=dev)
    z = torch.full((cap,), 123.0, dtype=torch.float32, device=dev)
    xy = torch.full((cap, 2), 55.0, dtype=torch.float32, device=dev)
    p = pkg.RGBDParams(500.0, 500.0, 8.0, 2.0, [0, 0, 0, 0, 0], 40.0, depth_scale=scale)
    pkg.rgbd_depth_batch_device(0, dk.data_ptr(), dn.data_ptr(), cap, 1, ddep.data_ptr(), 0, w * 4, w, h, p, pkg.DEPTH_F32, ur.data_ptr(),
                                z.data_ptr(), xy.data_ptr())
    torch.cuda.synchronize()
    n = len(xs)
    gur, gz, gxy = ur.cpu().numpy(), z.cpu().numpy(), xy.cpu().numpy()
    eur, ez = restate(xs, ys, xs, raw, f32(scale), 40.0)
    assert (_u32(gur[:n]) == _u32(eur)).all(), np.nonzero(_u32(gur[:n]) != _u32(eur))[0][:8]
    assert (_u32(gz[:n]) == _u32(ez)).all()
    assert gxy[:n].tobytes() == np.stack([xs, ys], 1).tobytes()             # dist_coef[0] == 0: kpU = kp
    assert (gur[n:] == 123).all() and (gz[n:] == 123).all() and (gxy[n:] == 55).all()
    assert np.isneginf(gur[:n]).any() and (gur[:n] == xs).any()           # denormal -> -inf, +inf -> kpU.x
    assert (gur[n - 9:n] == -1).sum() >= 6                                 # the out-of-image positions


@pytest.mark.gpu
def test_refusals_with_handle(pkg):
    ex = _ex(pkg)
    L = pkg.lib()
    p = params(pkg, TUM1)
    img = synth.image(3, W, H)
    raw = _depth_u16(3)
    cap = ex.max_keypoints(W, H)
    k = np.zeros(cap, pkg.KP_DTYPE); d = np.zeros((cap, 32), np.uint8); ur = np.zeros(cap, f32); z = np.zeros(cap, f32)
    n = C.c_int()

    def call(s, capacity=cap, dstride=W * 2, ch=1, dep=raw):
        return L.orbx_extract_rgbd(ex._h, img.ctypes.data, W, H, W * ch, ch, 1, dep.ctypes.data if dep is not None else None, dstride, C.byref(s),
                                   k.ctypes.data, d.ctypes.data, capacity, C.byref(n), None, ur.ctypes.data, z.ctypes.data)
    s = p.struct(pkg.DEPTH_U16)
    assert call(s) == 0 and n.value > 0
    assert call(s, capacity=cap - 1) == -2                    # ORBX_E_CAPACITY
    assert call(s, dstride=W * 2 - 2) == -1 and call(s, dstride=W * 2 + 1) == -1 and call(s, dep=None) == -1 and call(s, ch=2) == -1
    bad = p.struct(5)
    assert call(bad) == -1
    s3 = p.struct(pkg.DEPTH_U16); s3.ndist = 3
    assert call(s3) == -1
    t = C.c_int()
    assert L.orbx_extract_rgbd_submit(ex._h, img.ctypes.data, W, H, W, 1, 1, raw.ctypes.data, W * 2 - 2, C.byref(s), C.byref(t)) == -1
    ex1 = pkg.ORBextractor(NF, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=1)
    assert L.orbx_extract_rgbd_submit(ex1._h, img.ctypes.data, W, H, W, 1, 1, raw.ctypes.data, W * 2, C.byref(s), C.byref(t)) == -1


def _frames(n, seed0):
    out = []
    for i in range(n):
        ch = (1, 3, 4)[i % 3]
        img = synth.image(seed0 + i, W, H) if ch == 1 else _colour(seed0 + i, ch)
        raw = _depth_u16(seed0 + i) if i % 2 == 0 else _depth_f32(seed0 + i)
        out.append((img, raw, bool(i % 4 != 3)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("pinned", [False, True])
def test_pipelined(pkg, gather, pinned):
    """twelve frames with 1..4 in flight, RGB-D tickets interleaved with mono and stereo tickets on one handle; each result == the one-call
    form; both depth transports (ORBX_PIPE_RGBD_GATHER at handle creation); a wait through the wrong form is refused"""
    old = os.environ.get("ORBX_PIPE_RGBD_GATHER")
    os.environ["ORBX_PIPE_RGBD_GATHER"] = "1" if gather else "0"
    try:
        ex = _ex(pkg)
    finally:
        if old is None:
            os.environ.pop("ORBX_PIPE_RGBD_GATHER")
        else:
            os.environ["ORBX_PIPE_RGBD_GATHER"] = old
    one = _ex(pkg)
    p = params(pkg, TUM1)
    frames = _frames(12, 500)
    if pinned:
        pf = []
        for img, raw, rgb in frames:
            a = pkg.orbx.pinned_array(img.shape, np.uint8); a[...] = img
            b = pkg.orbx.pinned_array(raw.shape, raw.dtype); b[...] = raw
            pf.append((a, b, rgb))
        frames = pf
    exp = [one.extract_rgbd(img, raw, p, rgb=rgb) for img, raw, rgb in frames]
    mono_img = synth.image(900, W, H)
    l, r, _ = synth.stereo_pair(901, W, H)
    exp_mono = one(mono_img)
    bf, mz = 386.1448, 386.1448 / 718.856
    exp_st = one.extract_stereo(l, r, bf, mz)
    for depth in (1, 2, 3, 4):
        q, got = [], {}
        for i, (img, raw, rgb) in enumerate(frames):
            q.append(("rgbd", i, ex.extract_rgbd_submit(img, raw, p, rgb=rgb)))
            if i % 5 == 1 and len(q) < depth:
                q.append(("mono", None, ex.extract_submit(mono_img)))
            if i % 5 == 3 and len(q) < depth:
                q.append(("stereo", None, ex.extract_stereo_submit(l, r, bf, mz)))
            while len(q) >= depth:
                kind, j, t = q.pop(0)
                if kind == "rgbd":
                    got[j] = ex.extract_rgbd_wait(t)
                elif kind == "mono":
                    k, d = ex.extract_wait(t)
                    assert k.tobytes() == exp_mono[0].tobytes() and d.tobytes() == exp_mono[1].tobytes()
                else:
                    res = ex.extract_stereo_wait(t)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(res, exp_st))
        for kind, j, t in q:
            assert kind == "rgbd"
            got[j] = ex.extract_rgbd_wait(t)
        for i in range(len(frames)):
            _check_frame(f"depth {depth} frame {i}", got[i], exp[i])
    # the wrong form is refused and leaves the ticket valid
    t = ex.extract_rgbd_submit(frames[0][0], frames[0][1], p, rgb=frames[0][2])
    with pytest.raises(pkg.OrbxError):
        ex.extract_wait(t)
    with pytest.raises(pkg.OrbxError):
        ex.extract_stereo_wait(t)
    _check_frame("after refusals", ex.extract_rgbd_wait(t), exp[0])
    t = ex.extract_submit(mono_img)
    with pytest.raises(pkg.OrbxError):
        ex.extract_rgbd_wait(t)
    k, d = ex.extract_wait(t)
    assert k.tobytes() == exp_mono[0].tobytes()


def _batch_inputs(B, seed0):
    imgs, raws = [], []
    for i in range(B):
        img = synth.image(seed0 + i, W, H)
        if i == 2:
            img = np.full((H, W), 90, np.uint8)       # no keypoints
        if i == 4:
            flat = np.full((H, W), 60, np.uint8); flat[100:220, 300:460] = img[100:220, 300:460]; img = flat
        imgs.append(img)
        raws.append(_depth_u16(seed0 + 100 + i))
    return imgs, raws


def _run_batch(pkg, ex, imgs, raws, p, sp, with_xy=True):
    import torch
    dev = torch.device("cuda", 0)
    B = len(imgs)
    pitch = (W + 63) // 64 * 64
    host = np.zeros((B, H, pitch), np.uint8)
    for i, im in enumerate(imgs):
        host[i, :, :W] = im
    dpitch = W * 2 + 128                                   # padded rows: the pitch is honoured
    dhost = np.zeros((B, H, dpitch // 2), np.uint16)
    for i, r in enumerate(raws):
        dhost[i, :, :W] = r
    t_img = torch.from_numpy(host).to(dev); t_dep = torch.from_numpy(dhost).to(dev)
    cap = ex.max_keypoints(W, H)
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros(B, dtype=torch.int32, device=dev)
    ur = torch.full((B, cap), 123.0, dtype=torch.float32, device=dev)
    z = torch.full((B, cap), 321.0, dtype=torch.float32, device=dev)
    xy = torch.full((B, cap, 2), 55.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(t_img.data_ptr(), H * pitch, pitch, B, W, H, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), sp)
    pkg.rgbd_depth_batch_device(0, kps.data_ptr(), nout.data_ptr(), cap, B, t_dep.data_ptr(), H * dpitch, dpitch, W, H, p, pkg.DEPTH_U16,
                                ur.data_ptr(), z.data_ptr(), xy.data_ptr() if with_xy else None, sp)
    return dict(t_img=t_img, t_dep=t_dep, kps=kps, desc=desc, nout=nout, ur=ur, z=z, xy=xy, cap=cap)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 7, 32])
def test_batched_device(pkg, B):
    """extract_batch_device -> rgbd_depth_batch_device on a torch stream, differing counts (an image without keypoints): every image ==
    the one-call form; entries at or beyond a count stay untouched"""
    import torch
    ex = _ex(pkg, max_batch=B)
    one = _ex(pkg)
    p = params(pkg, TUM1)
    imgs, raws = _batch_inputs(B, 700 + B)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    r = _run_batch(pkg, ex, imgs, raws, p, stream.cuda_stream)
    ex.sync(stream.cuda_stream)
    stream.synchronize()
    n = r["nout"].cpu().numpy()
    ur, z, xy = r["ur"].cpu().numpy(), r["z"].cpu().numpy(), r["xy"].cpu().numpy()
    kps = r["kps"].cpu().numpy()
    for i in range(B):
        e = one.extract_rgbd(imgs[i], raws[i], p)
        m = int(n[i])
        assert m == len(e[0]), (i, m, len(e[0]))
        assert kps[i, :m].copy().view(pkg.KP_DTYPE).reshape(m).tobytes() == e[0].tobytes()
        assert xy[i, :m].tobytes() == e[2].tobytes(), i
        assert (_u32(ur[i, :m]) == _u32(e[3])).all() and (_u32(z[i, :m]) == _u32(e[4])).all(), i
        assert (ur[i, m:] == 123).all() and (z[i, m:] == 321).all() and (xy[i, m:] == 55).all(), i
    if B > 2:
        assert n[2] == 0 and n[4] < n[0]


@pytest.mark.gpu
def test_resident_rgbd_frame(pkg, oracle):
    """extract_batch_device -> rgbd_depth_batch_device -> DeviceFrame.from_extraction(d_u_right = the row, K, dist): read() == the one-call
    outputs; the three resident searches == their host-pointer twins == the oracle"""
    import torch
    from test_frame_resident import _check_all, _points_for
    ex = _ex(pkg, max_batch=2)
    one = _ex(pkg)
    p = params(pkg, TUM1)
    imgs, raws = _batch_inputs(2, 950)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    sp = stream.cuda_stream
    r = _run_batch(pkg, ex, imgs, raws, p, sp, with_xy=False)
    K = (TUM1["Camera.fx"], TUM1["Camera.fy"], TUM1["Camera.cx"], TUM1["Camera.cy"])
    bounds = (0.0, 0.0, float(W), float(H))
    cap = r["cap"]
    for b in range(2):
        df = pkg.DeviceFrame.from_extraction(0, r["kps"].data_ptr(), r["desc"].data_ptr(), r["nout"].data_ptr(), cap, b,
                                             d_u_right=r["ur"].data_ptr() + 4 * cap * b, K=K, dist_coef=p.dist_coef, bounds=bounds, stream=sp)
        e = one.extract_rgbd(imgs[b], raws[b], p)
        f = df.read()
        assert df.n == len(e[0]) > 500
        assert f["x"].tobytes() == np.ascontiguousarray(e[2][:, 0]).tobytes() and f["y"].tobytes() == np.ascontiguousarray(e[2][:, 1]).tobytes()
        assert f["u_right"].tobytes() == e[3].tobytes() and (f["u_right"] >= 0).sum() > 300
        assert f["desc"].tobytes() == e[1].tobytes() and f["octave"].tobytes() == e[0]["octave"].tobytes()
        cur = dict(f, occupied=np.zeros(df.n, np.uint8), bounds=bounds)
        pts = _points_for(cur, 31 + b)
        _check_all(pkg, oracle, df, cur, pts, ex.GetScaleFactors(), f"rgbd {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,padded", [("u16", False), ("u16", True), ("f32", False), ("f32", True)])
def test_adaptor_driver(pkg, tmp_path, dtype, padded):
    """ORBextractor::ExtractRGBD on CV_16U / CV_32F Mats, continuous and not: the vectors equal the one-call form"""
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"] + _compile_flags() +
                          [os.path.join(ROOT, "tests", "adapter_rgbd_driver.cc"), os.path.join(ROOT, "adapter", "ORBextractor.cc"),
                           os.path.join(ROOT, "adapter", "ORBextractor_rgbd.cc"), "-L", os.path.dirname(pkg.lib_path()), "-lorbx",
                           "-Wl,-rpath," + os.path.dirname(pkg.lib_path()), "-o", exe])
    img = synth.image(61, W, H)
    raw = _depth_u16(61) if dtype == "u16" else _depth_f32(61)
    (tmp_path / "g.raw").write_bytes(img.tobytes()); (tmp_path / "d.raw").write_bytes(raw.tobytes())
    p = params(pkg, TUM1)
    out = str(tmp_path / "out.bin")
    args = [exe, str(tmp_path / "g.raw"), str(tmp_path / "d.raw"), str(W), str(H), dtype, str(int(padded)), repr(float(p.depth_scale)),
            repr(float(p.bf)), repr(float(p.fx)), repr(float(p.fy)), repr(float(p.cx)), repr(float(p.cy)), "5"] + \
        [repr(float(v)) for v in p.dist_coef] + [out]
    subprocess.check_call(args, timeout=120)
    b = open(out, "rb").read()
    n = int(np.frombuffer(b[:4], np.int32)[0])
    o = 4
    keys = np.frombuffer(b[o:o + 28 * n], pkg.KP_DTYPE); o += 28 * n
    keysUn = np.frombuffer(b[o:o + 28 * n], pkg.KP_DTYPE); o += 28 * n
    desc = np.frombuffer(b[o:o + 32 * n], np.uint8).reshape(n, 32); o += 32 * n
    ur = np.frombuffer(b[o:o + 4 * n], f32); o += 4 * n
    z = np.frombuffer(b[o:o + 4 * n], f32)
    e = _ex(pkg).extract_rgbd(img, raw, p)
    assert n == len(e[0]) > 500 and keys.tobytes() == e[0].tobytes() and desc.tobytes() == e[1].tobytes()
    assert keysUn["x"].tobytes() == np.ascontiguousarray(e[2][:, 0]).tobytes() and keysUn["y"].tobytes() == np.ascontiguousarray(e[2][:, 1]).tobytes()
    assert keysUn["angle"].tobytes() == keys["angle"].tobytes() and keysUn["octave"].tobytes() == keys["octave"].tobytes()
    assert (_u32(ur) == _u32(e[3])).all() and (_u32(z) == _u32(e[4])).all()


@pytest.mark.gpu
def test_example_stream(pkg, tmp_path):
    """examples/rgbd_stream.c builds against the header and runs a short stream"""
    exe = str(tmp_path / "rgbd_stream")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rgbd_stream.c"),
                           "-L", os.path.dirname(pkg.lib_path()), "-lorbx", "-Wl,-rpath," + os.path.dirname(pkg.lib_path()), "-o", exe])
    res = subprocess.run([exe, "--frames", "40", "--channels", "3"], capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stderr
    j = json.loads(res.stdout.strip().splitlines()[-1])
    assert j["in_flight_1"]["frames_per_s"] > 0 and j["in_flight_4"]["frames_per_s"] > 0 and j["valid_depth_per_frame"] > 100
