"""Frame::isInFrustum + MapPoint::PredictScale (reference src/Frame.cc:310-380, src/MapPoint.cc) restated in numpy float32 / float64
scalars, one operation at a time, in the order include/orbx.h fixes for orbx_mappoints_frustum.  Independent of the library: the scale
level is ceil(logf(ratio) / lsf) evaluated directly with the C library's logf (through ctypes -- np.log on float32 is a different
function and disagrees with logf in the last bit on a fifth of all inputs), not through the library's threshold table.
level_thresholds() restates the table only for the tests that place points on its entries."""
import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    return f32(_libm.logf(float(f32(x))))


def level_of(ratio, lsf, nlevels):
    """clamp(ceilf(logf(ratio) / lsf), 0, nlevels - 1); a NaN ratio gives 0"""
    ratio = f32(ratio)
    if np.isnan(ratio):
        return 0
    with np.errstate(all="ignore"):
        q = np.ceil(f32(logf(ratio) / f32(lsf)))
    if np.isnan(q) or q < 0:
        return 0
    return int(min(q, nlevels - 1))


def level_predicate(r, lsf, k):
    """ceilf(logf(r) / lsf) > k, the predicate the library bisects"""
    with np.errstate(all="ignore"):
        return bool(np.ceil(f32(logf(r) / f32(lsf))) > k)


def bits(x):
    return int(np.array(x, f32).view(np.uint32))


def from_bits(b):
    return f32(np.array(b, np.uint32).view(f32))


def level_thresholds(lsf, nlevels):
    """r_k, k = 0 .. nlevels - 2: the smallest positive float with level_predicate(r, lsf, k)"""
    out = []
    for k in range(nlevels - 1):
        lo, hi = 0, 0x7F800000
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if level_predicate(from_bits(mid), lsf, k):
                hi = mid
            else:
                lo = mid
        out.append(from_bits(hi))
    return np.array(out, f32)


def frustum_point(g, pose, cam, view_cos_limit, lsf, nlevels):
    """one point: g = X Y Z dmin nx ny nz dmax -> None (not in view) or (u, v, xr, level, view_cos)"""
    X, Y, Z, dmin, nx, ny, nz, dmax = [f32(v) for v in g]
    R = [f32(v) for v in pose[:9]]; t = [f32(v) for v in pose[9:12]]; Ow = [f32(v) for v in pose[12:15]]
    fx, fy, cx, cy, mbf, mnx, mny, mxx, mxy = [f32(v) for v in cam]
    with np.errstate(all="ignore"):
        pc = [f32(f32(f32(f32(R[3 * k] * X) + f32(R[3 * k + 1] * Y)) + f32(R[3 * k + 2] * Z)) + t[k]) for k in range(3)]
        if pc[2] < f32(0):
            return None
        invz = f32(f32(1) / pc[2])
        u = f32(f32(f32(fx * pc[0]) * invz) + cx)
        v = f32(f32(f32(fy * pc[1]) * invz) + cy)
        if u < mnx or u > mxx or v < mny or v > mxy:
            return None
        if not (np.isfinite(u) and np.isfinite(v)):
            return None
        po = [f32(X - Ow[0]), f32(Y - Ow[1]), f32(Z - Ow[2])]
        d2 = f64(f64(f64(po[0]) * f64(po[0])) + f64(f64(po[1]) * f64(po[1]))) + f64(f64(po[2]) * f64(po[2]))
        dist = f32(np.sqrt(f64(d2)))
        if dist < f32(f32(0.8) * dmin) or dist > f32(f32(1.2) * dmax):
            return None
        dot = f64(f64(f64(po[0]) * f64(nx)) + f64(f64(po[1]) * f64(ny))) + f64(f64(po[2]) * f64(nz))
        vc = f32(f64(dot) / f64(dist))
        if not np.isfinite(vc) or vc < f32(view_cos_limit):
            return None
        ratio = f32(dmax / dist)
        level = level_of(ratio, lsf, nlevels)
        xr = f32(u - f32(mbf * invz))
    return u, v, xr, level, vc


def frustum(geom, eligible, pose, cam, view_cos_limit, lsf, nlevels):
    """all points -> dict(in_view, u, v, xr, level, view_cos); a point not in view (or not eligible) reads 0 everywhere"""
    n = len(geom)
    o = dict(in_view=np.zeros(n, np.uint8), u=np.zeros(n, f32), v=np.zeros(n, f32), xr=np.zeros(n, f32), level=np.zeros(n, np.int32),
             view_cos=np.zeros(n, f32))
    for i in range(n):
        if not eligible[i]:
            continue
        r = frustum_point(geom[i], pose, cam, view_cos_limit, lsf, nlevels)
        if r is None:
            continue
        o["in_view"][i] = 1
        o["u"][i], o["v"][i], o["xr"][i], o["level"][i], o["view_cos"][i] = r
    return o
