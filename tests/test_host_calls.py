"""The synchronous host-pointer entry points (orbx_hostapi.hip: orbx_extract, orbx_extract_batch, orbx_extract_color, orbx_extract_rectified,
orbx_extract_stereo, orbx_extract_rgbd) share one handle's staging buffers and one host-call path.  Two properties that no per-form parity
test sees: (1) every form interleaved on ONE handle, over image sizes that make the shared buffers grow, go unused and get reused, gives what
a fresh handle of exactly that size gives; (2) which check refuses a bad call, with which code and message, and that a refused call leaves
nothing half-staged."""
import ctypes as C

import numpy as np
import pytest

from tools import synth
from test_remap import _maps

CFG = (300, 1.2, 4, 20, 7)
MAX_SIZE = (320, 240)
SIZES = [(160, 120), (320, 240), (203, 131), (160, 120)]     # grow, (a smaller user in between), reuse
BF, MIN_Z = 40.0, 0.5
OK, E_INVALID, E_CAPACITY, E_TOO_SMALL = 0, -1, -2, -3


def _view(img, pad):
    """the same pixels as a view of a wider array: stride > width"""
    if not pad:
        return img
    buf = np.full((img.shape[0], img.shape[1] + pad), 201, np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


def _inputs(pkg, w, h):
    ns = w * h // 300 + 50
    pad = 29 if w % 4 else 0                                  # 203 x 131: width no multiple of 4 or 64, rows 232 bytes apart
    a, b, c, d = (synth.image(5 + k, w, h, nshapes=ns) for k in range(4))
    right = np.roll(a, -6, axis=1)                            # a constant disparity of 6 px: the stereo matcher finds matches
    rng = np.random.Generator(np.random.PCG64(w))
    dep16 = rng.integers(2500, 30000, (h, w)).astype(np.uint16)
    dep16[rng.random((h, w)) < 0.08] = 0
    dep32 = rng.uniform(0.3, 6.0, (h, w)).astype(np.float32)
    dep32[rng.random((h, w)) < 0.05] = 0
    mx, my = _maps(w, w, h, w, h)
    return dict(a=_view(a, pad), b=b, left=_view(a, pad), right=_view(right, pad), rgb=np.stack([a, b, c], 2), rgba=np.stack([a, b, c, d], 2),
                dep16=dep16, dep32=dep32, rect=pkg.Rectifier((w, h), mx, my),
                par=pkg.RGBDParams(210.0, 205.0, w / 2 + 1.5, h / 2 - 2.5, [0.12, -0.21, 0.001, 0.0007, 0.05], BF, DepthMapFactor=5000.0))


def _pipelined_stereo(ex, i):
    return ex.extract_stereo_wait(ex.extract_stereo_submit(i["left"], i["right"], BF, MIN_Z))


CALLS = [   # in the order of the issue: the 4-channel RGB-D call (the largest pinned input) before the stereo call (a smaller one)
    ("gray", lambda ex, i: ex(i["a"])),
    ("batch", lambda ex, i: ex.extract_batch([i["a"], i["b"]])),
    ("color3", lambda ex, i: ex.extract_color(i["rgb"], rgb=True, want_gray=True)),
    ("color4", lambda ex, i: ex.extract_color(i["rgba"], rgb=False, want_gray=True)),
    ("rgbd4_f32", lambda ex, i: ex.extract_rgbd(i["rgba"], i["dep32"], i["par"], rgb=True)),
    ("stereo", lambda ex, i: ex.extract_stereo(i["left"], i["right"], BF, MIN_Z)),
    ("stereo_pipelined", _pipelined_stereo),
    ("rgbd1_u16", lambda ex, i: ex.extract_rgbd(i["a"], i["dep16"], i["par"])),
    ("rectified", lambda ex, i: ex.extract_rectified(i["rect"], i["a"], want_rect=True)),
]


def _flat(res):
    if isinstance(res, np.ndarray):
        return [(res.dtype.str, res.shape, np.ascontiguousarray(res).tobytes())]
    return [x for r in res for x in _flat(r)]


@pytest.mark.gpu
def test_one_handle_every_form_interleaved(pkg, oracle):
    shared = pkg.ORBextractor(*CFG, device=0, max_size=MAX_SIZE, max_batch=2)
    orc = oracle.Oracle(*CFG)
    fresh, inputs = {}, {}
    for w, h in SIZES:
        if (w, h) not in inputs:
            inputs[w, h] = i = _inputs(pkg, w, h)
            assert i["a"].strides[0] >= w and (w % 4 == 0 or i["a"].strides[0] > w)
            # every call on a handle of its own, created for exactly this size
            fresh[w, h] = {name: _flat(fn(pkg.ORBextractor(*CFG, device=0, max_size=(w, h), max_batch=2), i)) for name, fn in CALLS}
        i = inputs[w, h]
        got = {}
        for name, fn in CALLS:
            res = fn(shared, i)
            got[name] = res
            assert _flat(res) == fresh[w, h][name], (w, h, name)
        oa = _flat(orc.extract(np.ascontiguousarray(i["a"]))); ob = _flat(orc.extract(i["b"]))
        assert len(got["gray"][0]) > 250, (w, h, len(got["gray"][0]))
        assert _flat(got["gray"]) == oa, (w, h)
        assert _flat(got["batch"][0]) == oa and _flat(got["batch"][1]) == ob, (w, h)
        assert _flat(got["stereo"][:2]) == oa and _flat(got["stereo_pipelined"][:2]) == oa, (w, h)
        assert (got["stereo"][4] >= 0).sum() > 20, (w, h)      # the stereo matcher had work
        assert _flat(got["rgbd1_u16"][:2]) == oa, (w, h)


def _err(L):
    return L.orbx_last_error().decode(errors="replace")


@pytest.mark.gpu
def test_host_call_error_contract(pkg, oracle):
    L = pkg.lib()
    ex = pkg.ORBextractor(*CFG, device=0, max_size=MAX_SIZE, max_batch=2)
    ex1 = pkg.ORBextractor(*CFG, device=0, max_size=MAX_SIZE, max_batch=1)
    w, h = 160, 120
    ns = w * h // 300 + 50
    a, b = synth.image(5, w, h, nshapes=ns), synth.image(6, w, h, nshapes=ns)
    rgb = np.stack([a, b, a], 2)
    dep = np.full((h, w), 1.5, np.float32)
    need = ex.max_keypoints(w, h)
    kps = np.zeros((2, need), pkg.KP_DTYPE); desc = np.zeros((2, need, 32), np.uint8); n = np.full(2, -7, np.int32)
    ur = np.zeros(need, np.float32); z = np.zeros(need, np.float32); xy = np.zeros((need, 2), np.float32)
    gray = np.zeros((h, w), np.uint8)
    mx, my = _maps(3, w, h, w, h)
    rect = pkg.Rectifier((w, h), mx, my)
    par = pkg.RGBDParams(210.0, 205.0, 80.0, 60.0, [0.1, -0.2, 0.0, 0.0], BF, depth_scale=1.0).struct(pkg.DEPTH_F32)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    small = synth.image(7, 97, 75, nshapes=80)

    def batch(batch=2, w=w, h=h, stride=w, cap=need, imgs=None, eh=ex):
        ptrs = (C.c_void_p * 3)(*(imgs if imgs is not None else [a.ctypes.data, b.ctypes.data, a.ctypes.data]))
        return L.orbx_extract_batch(eh._h, ptrs, batch, w, h, stride, p(kps), p(desc), cap, p(n))

    def color(w=w, h=h, stride=3 * w, channels=3, cap=need, gray_out=None, gray_stride=0):
        return L.orbx_extract_color(ex._h, p(rgb), w, h, stride, channels, 1, p(kps), p(desc), cap, n.ctypes.data_as(C.POINTER(C.c_int)),
                                    gray_out, gray_stride)

    def rectified(w=w, cap=need):
        return L.orbx_extract_rectified(ex._h, rect._h, p(a), w, h, w, p(kps), p(desc), cap, n.ctypes.data_as(C.POINTER(C.c_int)), None, 0)

    def stereo(w=w, cap=need, min_z=MIN_Z, eh=ex):
        return L.orbx_extract_stereo(eh._h, p(a), p(b), w, h, w, BF, min_z, p(kps), p(desc), cap, p(n), p(ur), p(z))

    def rgbd(w=w, cap=need):
        return L.orbx_extract_rgbd(ex._h, p(a), w, h, w, 1, 1, p(dep), 4 * w, C.byref(par), p(kps), p(desc), cap,
                                   n.ctypes.data_as(C.POINTER(C.c_int)), p(xy), p(ur), p(z))

    def refused(rc, code, text):
        assert rc == code and text in _err(L), (rc, _err(L), code, text)

    # orbx_extract_batch
    refused(batch(batch=0), E_INVALID, "orbx_extract_batch: invalid argument")
    refused(batch(batch=3), E_INVALID, "orbx_extract_batch: invalid argument")
    assert batch(w=0, stride=0) == OK and (n == 0).all()          # the empty image comes before any stride check
    refused(batch(stride=w - 1), E_INVALID, "stride < width")
    assert L.orbx_extract_batch(ex._h, (C.c_void_p * 1)(small.ctypes.data), 1, 97, 75, 97, p(kps), p(desc), need, p(n)) == E_TOO_SMALL
    refused(batch(cap=need - 1), E_CAPACITY, "keypoint capacity")
    refused(batch(imgs=[a.ctypes.data, None, None]), E_INVALID, "imgs[1] is NULL")
    # orbx_extract
    refused(L.orbx_extract(ex._h, None, w, h, w, p(kps), p(desc), need, n.ctypes.data_as(C.POINTER(C.c_int))), E_INVALID, "img is NULL")
    # orbx_extract_color
    refused(color(channels=2), E_INVALID, "orbx_extract_color: invalid argument")
    n[:] = -7
    assert color(w=0) == OK and n[0] == 0
    refused(color(stride=3 * w - 1), E_INVALID, "bad image / stride")
    refused(color(gray_out=p(gray), gray_stride=w - 1), E_INVALID, "orbx_extract_color: invalid argument")
    # orbx_extract_rectified / _stereo / _rgbd: no empty-image form
    refused(rectified(w=0), E_INVALID, "orbx_extract_rectified: invalid argument")
    refused(stereo(w=0), E_INVALID, "orbx_extract_stereo: invalid argument")
    refused(rgbd(w=0), E_INVALID, "orbx_extract_rgbd: invalid argument")
    refused(stereo(eh=ex1), E_INVALID, "max_batch >= 2")
    refused(stereo(min_z=0.0), E_INVALID, "orbx_extract_stereo: invalid argument")
    refused(rectified(cap=need - 1), E_CAPACITY, "keypoint capacity")
    refused(stereo(cap=need - 1), E_CAPACITY, "keypoint capacity")
    refused(rgbd(cap=need - 1), E_CAPACITY, "keypoint capacity")
    # a refused call leaves nothing half-staged: the next valid call on the same handle is the oracle's
    k, d = ex(a)
    ok, od = oracle.Oracle(*CFG).extract(a)
    assert len(k) == len(ok) > 250 and k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes()
