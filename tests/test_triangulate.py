"""orbx_triangulate_pairs / orbx_frame_triangulate (k_triangulate, k_tri_resolve) against tests/triangulate_model.py: status bytes, n_new
and the BIT PATTERNS of x3d.  The per-thread arithmetic has no reduction, so there is no tolerance (as tests/test_mappoints.py for
k_frustum).  The scenes (tests/triangulate_scene.py) hold n2 in {1, 3, 20}, per-neighbour counts from {0, 1, 63, 64, 65, 257} with cap
equal to the count and larger, totals that are no multiple of 256, the four stereo mixes, raw positions that differ from the undistorted
ones, one frame shared by two neighbours' lists, and every status value of the contract."""
import numpy as np
import pytest

import triangulate_scene as ts

f32 = np.float32
NAMES = [s["name"] for s in ts.scenes()]


def _suite(name):
    return next((s, e) for s, e in ts.suite() if s["name"] == name)


def _same(s, got, exp):
    """status, x3d bits and n_new, over the rows' written parts"""
    (st, x, n), (est, ex, en) = got, exp
    for i in range(len(s["k2s"])):
        k = int(s["npairs"][i])
        if st[i, :k].tobytes() != est[i, :k].tobytes():
            j = int(np.nonzero(st[i, :k] != est[i, :k])[0][0])
            return f"neighbour {i} pair {j}: status {st[i, j]} != {est[i, j]}"
        if x[i, :k].tobytes() != ex[i, :k].tobytes():
            j = int(np.nonzero((x[i, :k].view(np.uint32) != ex[i, :k].view(np.uint32)).any(1))[0][0])
            return f"neighbour {i} pair {j} (status {st[i, j]}): x3d {x[i, j]} != {ex[i, j]}"
        if st[i, k:].any() or x[i, k:].any():
            return f"neighbour {i}: written behind its list"
    return None if n == en else f"n_new {n} != {en}"


def _host(pkg, s):
    return pkg.triangulate_pairs(s["k1"], s["v1"], s["k2s"], s["v2s"], s["pairs"], s["npairs"], s["sf"], s["sigma2"], s["ratio_factor"])


def _device_frame(pkg, k, with_depth=True):
    n = len(k["x"])
    rng = np.random.Generator(np.random.PCG64(n))
    df = pkg.DeviceFrame(dict(x=k["x"], y=k["y"], octave=k["octave"], angle=rng.uniform(0, 360, n).astype(f32), u_right=k["u_right"],
                              desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), bounds=(-2000.0, -2000.0, 3000.0, 3000.0)))
    if with_depth:
        pkg.frame_set_depth(df, k["depth"], k["raw_x"], k["raw_y"])
    return df


def _resident(pkg, s, frames=None):
    made = {}
    def frame(k):   # one handle per keyframe, shared where the scene shares it
        if id(k) not in made:
            made[id(k)] = _device_frame(pkg, k)
        return made[id(k)]
    f1, f2 = frame(s["k1"]), [frame(k) for k in s["k2s"]]
    if frames is not None:
        frames.extend([f1] + f2)
    return pkg.frame_triangulate(f1, s["v1"], f2, s["v2s"], s["pairs"], s["npairs"], s["sf"], s["sigma2"], s["ratio_factor"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_matches_the_model(pkg, name):
    s, exp = _suite(name)
    got = _host(pkg, s)
    assert _same(s, got, exp) is None, _same(s, got, exp)
    assert _same(s, _host(pkg, s), exp) is None   # the staging is reused: a second call gives the same bytes


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_resident_equals_host_pointers(pkg, name):
    s, exp = _suite(name)
    frames = []
    got = _resident(pkg, s, frames)
    assert _same(s, got, _host(pkg, s)) is None and _same(s, got, exp) is None
    if name == "shared_frame":
        assert frames[1] is frames[3]


@pytest.mark.gpu
def test_raw_positions_enter_the_stereo_points(pkg):
    """UnprojectStereo reads mvKeys, everything else mvKeysUn: dropping the raw positions moves exactly the points made from a depth"""
    s, exp = _suite("raw_positions")
    plain = dict(s, k1=dict(s["k1"], raw_x=None, raw_y=None), k2s=[dict(k, raw_x=None, raw_y=None) for k in s["k2s"]])
    st, x, _ = _host(pkg, plain)
    moved = (x.view(np.uint32) != exp[1].view(np.uint32)).any(2)
    created = np.isin(exp[0], (1, 2, 33, 34))
    assert moved[created].all() and moved.sum() > 10
    assert not moved[np.isin(exp[0], (0, 32))].any()


@pytest.mark.gpu
def test_two_threads_share_the_frames(pkg):
    import threading
    s, exp = _suite("stereo_stereo")
    f1 = _device_frame(pkg, s["k1"]); f2 = [_device_frame(pkg, k) for k in s["k2s"]]
    res = [None, None]
    def run(t):
        for _ in range(3):
            res[t] = pkg.frame_triangulate(f1, s["v1"], f2, s["v2s"], s["pairs"], s["npairs"], s["sf"], s["sigma2"], s["ratio_factor"])
        pkg.lib().orbx_thread_release()
    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    [t.start() for t in th]; [t.join() for t in th]
    assert _same(s, res[0], exp) is None and _same(s, res[1], exp) is None


@pytest.mark.gpu
def test_frame_from_extraction(pkg):
    """a frame whose arrays exist on the device only: the first call waits for the creation; without depth it is refused; its octaves are
    checked by the kernel"""
    import torch
    s, exp = _suite("one_65")
    k = s["k1"]
    n, cap = len(k["x"]), 512
    kp = np.zeros((2, cap), pkg.KP_DTYPE)
    kp["x"][1, :n] = k["x"]; kp["y"][1, :n] = k["y"]; kp["octave"][1, :n] = k["octave"]; kp["size"][1, :n] = 31
    u = np.full((2, cap), 55.5, f32); u[1, :n] = k["u_right"]
    d = np.zeros((2, cap, 32), np.uint8)
    cnt = np.array([cap // 3, n], np.int32)
    dev = torch.device("cuda", 0)
    tk, td, tu, tn = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev) for a in (kp, d, u, cnt)]
    torch.cuda.synchronize()
    f1 = pkg.DeviceFrame.from_extraction(0, tk.data_ptr(), td.data_ptr(), tn.data_ptr(), cap, 1, d_u_right=tu.data_ptr() + 4 * cap,
                                         bounds=(-2000.0, -2000.0, 3000.0, 3000.0))
    f2 = [_device_frame(pkg, s["k2s"][0])]
    args = (s["v1"], f2, s["v2s"], s["pairs"], s["npairs"])
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.frame_triangulate(f1, *args, s["sf"], s["sigma2"], s["ratio_factor"])
    assert ei.value.code == -1 and "depth" in str(ei.value)
    pkg.frame_set_depth(f1, k["depth"])
    got = pkg.frame_triangulate(f1, *args, s["sf"], s["sigma2"], s["ratio_factor"])
    assert _same(s, got, exp) is None
    # two levels only, and pairs whose neighbour feature the host lets through (it knows keyframe 2's octaves): the level-2 features of
    # keyframe 1 among them are found by the kernel
    pr = s["pairs"][0, :2 * s["npairs"][0]].reshape(-1, 2)
    pr = pr[s["k2s"][0]["octave"][pr[:, 1]] <= 1]
    assert (k["octave"][pr[:, 0]] == 2).any()
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.frame_triangulate(f1, s["v1"], f2, s["v2s"], pr.reshape(1, -1), [len(pr)], s["sf"][:2], s["sigma2"][:2], s["ratio_factor"])
    assert ei.value.code == -1 and "octave" in str(ei.value)


@pytest.mark.gpu
def test_resident_refusals(pkg):
    s, _ = _suite("stereo_stereo")
    f1 = _device_frame(pkg, s["k1"], with_depth=False)
    f2 = [_device_frame(pkg, k) for k in s["k2s"]]
    call = lambda a, b: pkg.frame_triangulate(a, s["v1"], b, s["v2s"], s["pairs"], s["npairs"], s["sf"], s["sigma2"], s["ratio_factor"])
    with pytest.raises(pkg.OrbxError) as ei:     # stereo features, no depth attached
        call(f1, f2)
    assert ei.value.code == -1 and "depth" in str(ei.value)
    pkg.frame_set_depth(f1, s["k1"]["depth"])
    call(f1, f2)
    with pytest.raises(pkg.OrbxError):           # once per frame
        pkg.frame_set_depth(f1, s["k1"]["depth"])
    pr = s["pairs"].copy(); pr[0, 1] = ts.N1
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.frame_triangulate(f1, s["v1"], f2, s["v2s"], pr, s["npairs"], s["sf"], s["sigma2"], s["ratio_factor"])
    assert ei.value.code == -1 and "outside the keyframes" in str(ei.value)
    mono = _suite("mono_mono")[0]
    g1 = _device_frame(pkg, mono["k1"], with_depth=False)   # a monocular keyframe needs no depth
    g2 = [_device_frame(pkg, k, with_depth=False) for k in mono["k2s"]]
    got = pkg.frame_triangulate(g1, mono["v1"], g2, mono["v2s"], mono["pairs"], mono["npairs"], mono["sf"], mono["sigma2"], mono["ratio_factor"])
    assert _same(mono, got, _suite("mono_mono")[1]) is None
