"""The triangulation contract of include/orbx.h (orbx_triangulate_pairs) restated in numpy, one operation at a time on np.float32 /
np.float64 scalars, independent of the library: the body of LocalMapping::CreateNewMapPoints' match loop (reference
src/LocalMapping.cc:327-511) and the loop's order rule in two formulations.

A view is a dict(Tcw[3][4], Ow[3], fx, fy, cx, cy, invfx, invfy, mb, mbf) of float32; a keyframe a dict(x, y, octave, u_right, depth,
raw_x, raw_y) of arrays (depth / raw_x / raw_y may be None)."""
import numpy as np

F = np.float32
D = np.float64
EPS2 = D(F(2.0) * F(1.1920928955078125e-7))

CREATED = (0, 1, 2)
ST_LOW_PARALLAX, ST_W0, ST_Z1, ST_Z2, ST_REPROJ1, ST_REPROJ2, ST_DIST0, ST_SCALE, ST_NO_DEPTH = 16, 17, 18, 19, 20, 21, 22, 23, 24
SUPERSEDED = 32
ALL_STATUS = (0, 1, 2, 16, 17, 18, 19, 20, 21, 22, 23, 24, 32, 33, 34)


def dotd(a, b):
    return (D(a[0]) * D(b[0]) + D(a[1]) * D(b[1])) + D(a[2]) * D(b[2])


def rot_wc(T, v, add=(0.0, 0.0, 0.0)):
    """Rwc * v + add, Rwc the transpose of T's rotation block; one cast per row"""
    return [F(dotd((T[0][r], T[1][r], T[2][r]), v) + D(add[r])) for r in range(3)]


def cam_row(T, r, X):
    return F(dotd(T[r][:3], X) + D(T[r][3]))


def stereo_cos(mb, depth):
    h = D(F(mb) / F(2.0)); d = D(F(depth))
    return F((d * d - h * h) / (d * d + h * h))


def norm3(v):
    return F(np.sqrt(dotd(v, v)))


def matrix_A(xn1, xn2, T1, T2):
    A = np.zeros((4, 4), F)
    for c in range(4):
        A[0][c] = F(xn1[0] * T1[2][c]) - T1[0][c]
        A[1][c] = F(xn1[1] * T1[2][c]) - T1[1][c]
        A[2][c] = F(xn2[0] * T2[2][c]) - T2[0][c]
        A[3][c] = F(xn2[1] * T2[2][c]) - T2[1][c]
    return A


def null_vector(A):
    """one-sided Jacobi on the columns of the float A (the shape of OpenCV's JacobiSVDImpl_) -> the row of V of the smallest column"""
    At = [[F(A[k][i]) for k in range(4)] for i in range(4)]
    V = [[F(1.0) if i == k else F(0.0) for k in range(4)] for i in range(4)]
    W = []
    for i in range(4):
        sd = D(0.0)
        for k in range(4):
            sd = sd + D(At[i][k]) * D(At[i][k])
        W.append(sd)
    for _sweep in range(30):
        changed = False
        for i in range(3):
            for j in range(i + 1, 4):
                a, b, p = W[i], W[j], D(0.0)
                for k in range(4):
                    p = p + D(At[i][k]) * D(At[j][k])
                if abs(p) <= EPS2 * np.sqrt(a * b):
                    continue
                p = p * D(2.0)
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * D(0.5)
                    s = F(np.sqrt(delta / gamma))
                    c = F(p / ((gamma * D(s)) * D(2.0)))
                else:
                    c = F(np.sqrt((gamma + beta) / (gamma * D(2.0))))
                    s = F(p / ((gamma * D(c)) * D(2.0)))
                a = D(0.0); b = D(0.0)
                for k in range(4):
                    t0 = F(c * At[i][k]) + F(s * At[j][k])
                    t1 = F((-s) * At[i][k]) + F(c * At[j][k])
                    At[i][k] = t0; At[j][k] = t1
                    a = a + D(t0) * D(t0); b = b + D(t1) * D(t1)
                W[i] = a; W[j] = b
                for k in range(4):
                    t0 = F(c * V[i][k]) + F(s * V[j][k])
                    t1 = F((-s) * V[i][k]) + F(c * V[j][k])
                    V[i][k] = t0; V[j][k] = t1
                changed = True
        if not changed:
            break
    best, sel = None, 0
    for i in range(4):
        sd = D(0.0)
        for k in range(4):
            sd = sd + D(At[i][k]) * D(At[i][k])
        if i == 0 or sd <= best:
            best, sel = sd, i
    return V[sel]


def reproj_ok(v, X, z, kx, ky, ur, stereo, sigma2, mbf):
    T = v["Tcw"]
    x = cam_row(T, 0, X); y = cam_row(T, 1, X)
    invz = F(D(1.0) / D(z))
    u = F(F(v["fx"] * x) * invz) + v["cx"]
    w = F(F(v["fy"] * y) * invz) + v["cy"]
    ex = u - kx; ey = w - ky
    if not stereo:
        return not (D(F(ex * ex) + F(ey * ey)) > D(5.991) * D(sigma2))
    u_r = u - F(mbf * invz)
    er = u_r - ur
    return not (D(F(F(ex * ex) + F(ey * ey)) + F(er * er)) > D(7.8) * D(sigma2))


def unproject(v, kf, i):
    z = F(kf["depth"][i])
    if not (z > 0):
        return None
    rx = kf["raw_x"] if kf.get("raw_x") is not None else kf["x"]
    ry = kf["raw_y"] if kf.get("raw_y") is not None else kf["y"]
    x = F(F(F(rx[i]) - v["cx"]) * z) * v["invfx"]
    y = F(F(F(ry[i]) - v["cy"]) * z) * v["invfy"]
    return rot_wc(v["Tcw"], (x, y, z), v["Ow"])


def test_pair(v1, k1, i1, v2, k2, i2, sf, sigma2, ratio_factor, info=None):
    """-> (status, x3d[3] float32); info (a dict) receives A, the accepted parallax cosine, ..."""
    with np.errstate(all="ignore"):
        return _test_pair(v1, k1, i1, v2, k2, i2, sf, sigma2, F(ratio_factor), info)


def _test_pair(v1, k1, i1, v2, k2, i2, sf, sigma2, ratio_factor, info):
    zero = np.zeros(3, F)
    k1x, k1y, ur1 = F(k1["x"][i1]), F(k1["y"][i1]), F(k1["u_right"][i1])
    k2x, k2y, ur2 = F(k2["x"][i2]), F(k2["y"][i2]), F(k2["u_right"][i2])
    o1, o2 = int(k1["octave"][i1]), int(k2["octave"][i2])
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    T1, T2 = v1["Tcw"], v2["Tcw"]
    xn1 = (F(k1x - v1["cx"]) * v1["invfx"], F(k1y - v1["cy"]) * v1["invfy"], F(1.0))
    xn2 = (F(k2x - v2["cx"]) * v2["invfx"], F(k2y - v2["cy"]) * v2["invfy"], F(1.0))
    r1 = rot_wc(T1, xn1); r2 = rot_wc(T2, xn2)
    cos_rays = F(dotd(r1, r2) / (np.sqrt(dotd(r1, r1)) * np.sqrt(dotd(r2, r2))))
    cs1 = cos_rays + F(1.0); cs2 = cs1
    if st1:
        cs1 = stereo_cos(v1["mb"], k1["depth"][i1])
    elif st2:
        cs2 = stereo_cos(v2["mb"], k2["depth"][i2])
    cos_stereo = cs2 if cs2 < cs1 else cs1
    if info is not None:
        info["cos_rays"] = cos_rays
    if cos_rays < cos_stereo and cos_rays > 0 and (st1 or st2 or D(cos_rays) < D(0.9998)):
        A = matrix_A(xn1, xn2, T1, T2)
        if info is not None:
            info["A"] = A.copy()
        v = null_vector(A)
        if v[3] == 0:
            return ST_W0, zero
        X = [v[0] / v[3], v[1] / v[3], v[2] / v[3]]
        created = 0
    elif st1 and cs1 < cs2:
        X = unproject(v1, k1, i1)
        created = 1
    elif st2 and cs2 < cs1:
        X = unproject(v2, k2, i2)
        created = 2
    else:
        return ST_LOW_PARALLAX, zero
    if X is None:
        return ST_NO_DEPTH, zero
    x3d = np.array(X, F)
    z1 = cam_row(T1, 2, X)
    if z1 <= 0:
        return ST_Z1, x3d
    z2 = cam_row(T2, 2, X)
    if z2 <= 0:
        return ST_Z2, x3d
    if not reproj_ok(v1, X, z1, k1x, k1y, ur1, st1, F(sigma2[o1]), v1["mbf"]):
        return ST_REPROJ1, x3d
    if not reproj_ok(v2, X, z2, k2x, k2y, ur2, st2, F(sigma2[o2]), v1["mbf"]):   # :465: the current keyframe's mbf
        return ST_REPROJ2, x3d
    d1 = norm3([X[r] - v1["Ow"][r] for r in range(3)])
    d2 = norm3([X[r] - v2["Ow"][r] for r in range(3)])
    if d1 == 0 or d2 == 0:
        return ST_DIST0, x3d
    ratio_dist = d2 / d1
    ratio_oct = F(sf[o1]) / F(sf[o2])
    if ratio_dist * ratio_factor < ratio_oct or ratio_dist > ratio_oct * ratio_factor:
        return ST_SCALE, x3d
    return created, x3d


def _outputs(scene):
    n2, cap = len(scene["k2s"]), scene["cap"]
    return np.zeros((n2, cap), np.uint8), np.zeros((n2, cap, 3), F)


def _pair(scene, i, k):
    i1, i2 = int(scene["pairs"][i][2 * k]), int(scene["pairs"][i][2 * k + 1])
    st, x = test_pair(scene["v1"], scene["k1"], i1, scene["v2s"][i], scene["k2s"][i], i2, scene["sf"], scene["sigma2"], scene["ratio_factor"])
    return i1, st, x


def first_wins(scene):
    """test every pair on its own, then per idx1 keep the pair of the first neighbour whose tests pass -> status, x3d, n_new"""
    status, x3d = _outputs(scene)
    first = {}
    for i in range(len(scene["k2s"])):
        for k in range(int(scene["npairs"][i])):
            i1, st, x = _pair(scene, i, k)
            status[i][k] = st; x3d[i][k] = x
            if st in CREATED:
                first[i1] = min(first.get(i1, i), i)
    for i in range(len(scene["k2s"])):
        for k in range(int(scene["npairs"][i])):
            if status[i][k] in CREATED and i > first[int(scene["pairs"][i][2 * k])]:
                status[i][k] += SUPERSEDED
    return status, x3d, int(np.sum(status[_mask(scene)] <= 2))


def sequential(scene):
    """the reference's loop: neighbour by neighbour, a feature of keyframe 1 that got a point at an earlier neighbour is skipped by the
    later searches (src/ORBmatcher.cc:750-751).  A skipped pair never reaches the loop body: to stay comparable it is still tested and
    reads 32 + status if it would have been created, its own status otherwise."""
    status, x3d = _outputs(scene)
    has_point = set()
    for i in range(len(scene["k2s"])):
        created_here = set()
        for k in range(int(scene["npairs"][i])):
            i1, st, x = _pair(scene, i, k)
            x3d[i][k] = x
            if i1 in has_point:
                status[i][k] = st + SUPERSEDED if st in CREATED else st
                continue
            status[i][k] = st
            if st in CREATED:
                created_here.add(i1)
        has_point |= created_here   # the flags change between two searches, not within one
    return status, x3d, int(np.sum(status[_mask(scene)] <= 2))


def _mask(scene):
    n2, cap = len(scene["k2s"]), scene["cap"]
    m = np.zeros((n2, cap), bool)
    for i in range(n2):
        m[i, :int(scene["npairs"][i])] = True
    return m


def svd_null_point(A):
    """the float A's null vector by a float64 numpy.linalg.svd, dehomogenised in float64"""
    vt = np.linalg.svd(np.asarray(A, D))[2]
    v = vt[3]
    return v[:3] / v[3]
