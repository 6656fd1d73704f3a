"""The per-thread contexts of the per-call searches (ThreadCtx, orb-slam2_amd/csrc/orbx_internal.h): every family gives its
stream and staging back on orbx_thread_release and when its thread ends, sets them up again on the next call, grows and
reuses its buffers without changing a result, and refuses an unusable device with one message and no context left behind.
The four families: the per-call matcher (SearchByBoW, form "auto"), the legacy SearchByBoW kernels (form "wave"), the
projection search on host arrays, UndistortKeyPoints."""
import functools
import threading
import time

import numpy as np
import pytest

from test_matchers_percall import _scene
from test_projection import _scene as _proj_scene
from test_undistort import CAMS, _pts

RATIO, TH = 0.8, 3.0
FX, FY, CX, CY, DIST = CAMS[0]          # k1 != 0: the kernel runs


@functools.lru_cache(maxsize=None)
def _inputs(n, npts):
    """the inputs of one round of the four families: two keyframes + a frame of n features, npts projected points, n positions"""
    cur, kfs, *_ = _scene(300 + n, n, (n, n), k=10 if n >= 100 else 4)   # (the vocabulary takes k * k of the descriptors as its nodes)
    pcur, pts, sf = _proj_scene(400 + n, n, npts)
    pts = dict(pts); pts["aux"] = (pts["u"] - 5).astype(np.float32)
    return cur, kfs, pcur, pts, sf, _pts(500 + n, n)


@functools.lru_cache(maxsize=None)
def _expected(oracle, n, npts):
    """the oracle's results of that round, computed once and shared"""
    cur, kfs, pcur, pts, sf, xy = _inputs(n, npts)
    bow = [oracle.search_by_bow_kf_f(kf, cur, RATIO, True) for kf in kfs]
    return bow, oracle.search_by_projection_points(pcur, pts, sf, TH, RATIO), oracle.undistort_points(xy, FX, FY, CX, CY, DIST)


def _families(pkg, n, npts, device=0):
    """the four calls, in the order the docstring names the families"""
    cur, kfs, pcur, pts, sf, xy = _inputs(n, npts)
    m = pkg.ORBmatcher(RATIO, True, device=device)

    def legacy():
        pkg.orbx.debug_set_bow_form("wave")
        try:
            return [m.SearchByBoW(kf, cur) for kf in kfs]
        finally:
            pkg.orbx.debug_set_bow_form("auto")
    return (lambda: [m.SearchByBoW(kf, cur) for kf in kfs], legacy,
            lambda: m.SearchByProjectionMapPoints(pcur, pts, sf, TH),
            lambda: pkg.UndistortKeyPoints(xy, FX, FY, CX, CY, DIST, device=device))


def _round(pkg, oracle, n, npts):
    """runs the four families, checks each against the oracle, returns the results in a comparable form"""
    bow, legacy, proj, und = [f() for f in _families(pkg, n, npts)]
    ebow, eproj, eund = _expected(oracle, n, npts)
    for got in (bow, legacy):
        for (g, c), (e, ec) in zip(got, ebow):
            assert c == ec and (g == e).all()
    assert proj[1] == eproj[1] and (proj[0] == eproj[0]).all()
    assert und.tobytes() == eund.tobytes()
    return ([(g.tobytes(), c) for g, c in bow], [(g.tobytes(), c) for g, c in legacy], (proj[0].tobytes(), proj[1]), und.tobytes())


def _in_thread(fn):
    """runs fn in a thread of its own that ends without releasing anything; its exception, if any, is raised here"""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as exc:     # noqa: BLE001 (handed to the caller)
            box["error"] = exc
    t = threading.Thread(target=body)
    t.start(); t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def _settled(pkg, target):
    """the context count once it has reached `target`; the thread-end destructors may run just after join(), so wait for them, 2 s at most"""
    end = time.monotonic() + 2.0
    while pkg.orbx.debug_thread_contexts() != target and time.monotonic() < end:
        time.sleep(0.005)
    return pkg.orbx.debug_thread_contexts()


@pytest.mark.gpu
def test_release_and_reuse(pkg, oracle):
    count = pkg.orbx.debug_thread_contexts
    c0 = count()

    def worker():
        first = _round(pkg, oracle, 300, 200)
        assert count() == c0 + 4
        pkg.orbx.thread_release()
        assert count() == c0
        assert _round(pkg, oracle, 300, 200) == first
        assert count() == c0 + 4
    _in_thread(worker)
    assert _settled(pkg, c0) == c0


@pytest.mark.gpu
def test_many_short_lived_threads(pkg, oracle):
    c0 = pkg.orbx.debug_thread_contexts()
    results = [_in_thread(lambda: _round(pkg, oracle, 300, 200)) for _ in range(8)]
    assert all(r == results[0] for r in results[1:])
    assert _settled(pkg, c0) == c0


@pytest.mark.gpu
def test_growth_reuse_regrowth(pkg, oracle):
    """each size beyond twice the one before it (a block is allocated at twice the request), a small one in between on the larger block"""
    count = pkg.orbx.debug_thread_contexts
    c0 = count()

    def worker():
        for n, npts in ((64, 48), (1200, 900), (64, 48), (2500, 1900)):
            _round(pkg, oracle, n, npts)
            assert count() == c0 + 4, n
    _in_thread(worker)
    assert _settled(pkg, c0) == c0


def test_refusals(pkg):
    """runs with and without a GPU; in a thread of its own, so that the release at the end meets no context of earlier tests"""
    count = pkg.orbx.debug_thread_contexts
    devices = [-1, 16] + ([0] if pkg.orbx.lib().orbx_device_count() == 0 else [])
    c0 = count()

    def worker():
        for device in devices:
            messages = []
            for call in _families(pkg, 64, 48, device=device):
                with pytest.raises(pkg.OrbxError) as ei:
                    call()
                assert ei.value.code == -4
                messages.append(str(ei.value))
            assert messages == [f"orbx error -4: no usable HIP device {device} (liborbx has no CPU fallback)"] * 4
        assert count() == c0
        pkg.orbx.thread_release()
        assert count() == c0
    _in_thread(worker)
    assert count() == c0
