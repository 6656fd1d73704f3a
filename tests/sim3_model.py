"""The Sim3Solver contract of include/orbx.h (orbx_sim3_hypotheses) restated in numpy, one operation at a time on np.float32 / np.float64
scalars where the order matters (Horn's closed form, the Jacobi eigen-solver) and element-wise over the points in CheckInliers, where
every point is on its own.  It also holds Sim3Solver::iterate (reference src/Sim3Solver.cc:143-211) twice: `Replay` walks a finished table
of hypotheses as the adaptor does, `Sequential` is the literal loop that evaluates a hypothesis only when it reaches it."""
import math

import numpy as np

f = np.float32
d = np.float64
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
SWEEPS = 30


def threshold(sigma2):
    """mvnMaxError: push_back(9.210 * sigmaSquare) into a vector<size_t>, compared against a float"""
    return f(int(9.210 * float(f(sigma2))))


def dotd(a0, a1, a2, b0, b1, b2):
    return (d(a0) * d(b0) + d(a1) * d(b1)) + d(a2) * d(b2)


def hyp(a, b):
    return f(np.sqrt(d(a) * d(a) + d(b) * d(b)))


def _rot(M, i0, j0, i1, j1, c, s):
    a0, b0 = M[i0][j0], M[i1][j1]
    M[i0][j0] = a0 * c - b0 * s
    M[i1][j1] = a0 * s + b0 * c


def top_eigenvector(N, info=None):
    """N: 4 x 4 float32 (the upper triangle is read) -> q[4], the row of V of the largest W, of equal ones the earlier"""
    A = [[f(N[i][j]) for j in range(4)] for i in range(4)]
    V = [[f(1.0) if i == j else f(0.0) for j in range(4)] for i in range(4)]
    W = [A[i][i] for i in range(4)]
    sweeps = 0
    for _ in range(SWEEPS):
        changed = False
        sweeps += 1
        for k in range(3):
            for l in range(k + 1, 4):
                p = A[k][l]
                if d(p) * d(p) <= d(2.0 ** -46) * abs(d(W[k]) * d(W[l])):
                    continue
                changed = True
                y = (W[l] - W[k]) * f(0.5)
                t = abs(y) + hyp(p, y)
                s = hyp(p, t)
                c = t / s
                s = p / s
                t = (p / t) * p
                if y < f(0.0):
                    s, t = -s, -t
                A[k][l] = f(0.0)
                W[k] = W[k] - t
                W[l] = W[l] + t
                for i in range(k):
                    _rot(A, i, k, i, l, c, s)
                for i in range(k + 1, l):
                    _rot(A, k, i, i, l, c, s)
                for i in range(l + 1, 4):
                    _rot(A, k, i, l, i, c, s)
                for i in range(4):
                    _rot(V, k, i, l, i, c, s)
        if not changed:
            break
    best = 0
    for i in range(1, 4):
        if W[i] > W[best]:
            best = i
    if info is not None:
        info["sweeps"] = sweeps
        info["W"] = W
    return V[best]


def horn(P1, P2, fix_scale, info=None):
    """P1, P2: [3 points][3] float32 -> dict(deg, s, R[3][3], t[3], sR, sRi, t21) as float32 scalars"""
    with np.errstate(all="ignore"):
        p1 = [[f(P1[i][r]) for i in range(3)] for r in range(3)]   # [row][point]
        p2 = [[f(P2[i][r]) for i in range(3)] for r in range(3)]
        third = d(1.0) / d(3.0)
        O1 = [f(d((p1[r][0] + p1[r][1]) + p1[r][2]) * third) for r in range(3)]
        O2 = [f(d((p2[r][0] + p2[r][1]) + p2[r][2]) * third) for r in range(3)]
        Pr1 = [[p1[r][i] - O1[r] for i in range(3)] for r in range(3)]
        Pr2 = [[p2[r][i] - O2[r] for i in range(3)] for r in range(3)]
        M = [[f(dotd(*Pr2[r], *Pr1[c])) for c in range(3)] for r in range(3)]
        z0 = f(0.0)
        N = [[z0] * 4 for _ in range(4)]
        N[0][0] = (M[0][0] + M[1][1]) + M[2][2]
        N[0][1] = M[1][2] - M[2][1]
        N[0][2] = M[2][0] - M[0][2]
        N[0][3] = M[0][1] - M[1][0]
        N[1][1] = (M[0][0] - M[1][1]) - M[2][2]
        N[1][2] = M[0][1] + M[1][0]
        N[1][3] = M[2][0] + M[0][2]
        N[2][2] = ((-M[0][0]) + M[1][1]) - M[2][2]
        N[2][3] = M[1][2] + M[2][1]
        N[3][3] = ((-M[0][0]) - M[1][1]) + M[2][2]
        if info is not None:
            info["N"] = np.array([[N[min(i, j)][max(i, j)] for j in range(4)] for i in range(4)], f)
            info["O1"], info["O2"], info["Pr1"], info["Pr2"] = O1, O2, Pr1, Pr2
        q = top_eigenvector(N, info)
        deg = bool(q[1] == z0 and q[2] == z0 and q[3] == z0)
        w, x, y, z = d(q[0]), d(q[1]), d(q[2]), d(q[3])
        ww, xx, yy, zz, xy, xz, yz, wx, wy, wz = w * w, x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        n2 = ((ww + xx) + yy) + zz
        two = d(2.0)
        R = [[f((((ww + xx) - yy) - zz) / n2), f((two * (xy - wz)) / n2), f((two * (xz + wy)) / n2)],
             [f((two * (xy + wz)) / n2), f((((ww - xx) + yy) - zz) / n2), f((two * (yz - wx)) / n2)],
             [f((two * (xz - wy)) / n2), f((two * (yz + wx)) / n2), f((((ww - xx) - yy) + zz) / n2)]]
        s12 = f(1.0)
        if not fix_scale:
            nom, den = d(0.0), d(0.0)
            for r in range(3):
                for i in range(3):
                    p3 = f(dotd(*R[r], Pr2[0][i], Pr2[1][i], Pr2[2][i]))
                    nom = nom + d(Pr1[r][i]) * d(p3)
                    den = den + d(p3 * p3)
            s12 = f(nom / den)
        sd, si = d(s12), d(1.0) / d(s12)
        t12 = [f(d(O1[r]) - sd * dotd(*R[r], *O2)) for r in range(3)]
        sR = [[f(sd * d(R[r][c])) for c in range(3)] for r in range(3)]
        sRi = [[f(si * d(R[c][r])) for c in range(3)] for r in range(3)]
        t21 = [f(-dotd(*sRi[r], *t12)) for r in range(3)]
    return dict(deg=deg, s=s12, R=R, t=t12, sR=sR, sRi=sRi, t21=t21)


def _project(T, tv, X, K):
    """Project (:389-410) element-wise over X[n][3] float32 -> u[n], v[n]"""
    x0, x1, x2 = X[:, 0].astype(d), X[:, 1].astype(d), X[:, 2].astype(d)
    pc = [(((d(T[r][0]) * x0 + d(T[r][1]) * x1) + d(T[r][2]) * x2) + d(tv[r])).astype(f) for r in range(3)]
    return _to_image(pc[0], pc[1], pc[2], K)


def _to_image(X, Y, Z, K):
    invz = f(1.0) / Z
    x, y = X * invz, Y * invz
    return f(K[0]) * x + f(K[2]), f(K[1]) * y + f(K[3])


def _err(u0, v0, u1, v1):
    d0, d1 = u0 - u1, v0 - v1
    return (d0.astype(d) * d0.astype(d) + d1.astype(d) * d1.astype(d)).astype(f)


def check_inliers(job, h):
    """CheckInliers (:347-371) for the solution h of horn() -> bool[n]"""
    X1, X2 = np.ascontiguousarray(job["X1"], f), np.ascontiguousarray(job["X2"], f)
    K1, K2 = np.asarray(job["K1"], f), np.asarray(job["K2"], f)
    with np.errstate(all="ignore"):
        u11, v11 = _to_image(X1[:, 0], X1[:, 1], X1[:, 2], K1)
        u22, v22 = _to_image(X2[:, 0], X2[:, 1], X2[:, 2], K2)
        u21, v21 = _project(h["sR"], h["t"], X2, K1)
        u12, v12 = _project(h["sRi"], h["t21"], X1, K2)
        e1 = _err(u11, v11, u21, v21)
        e2 = _err(u12, v12, u22, v22)
        return (e1 < np.asarray(job["max_err1"], f)) & (e2 < np.asarray(job["max_err2"], f))


def hypothesis(job, sample):
    """one row of the table -> (n_inliers, srt[13] float32, inliers bool[n])"""
    X1, X2 = np.asarray(job["X1"], f), np.asarray(job["X2"], f)
    h = horn(X1[list(sample)], X2[list(sample)], job["fix_scale"])
    n = len(X1)
    if h["deg"]:
        return 0, np.full(13, QNAN, f), np.zeros(n, bool)
    inl = check_inliers(job, h)
    srt = np.array([h["s"]] + [h["R"][r][c] for r in range(3) for c in range(3)] + list(h["t"]), f)
    return int(inl.sum()), srt, inl


def pack_bits(inl):
    """bool[n] -> uint64[(n+63)/64], bit i % 64 of word i / 64"""
    n = len(inl)
    words = (n + 63) // 64
    pad = np.zeros(words * 64, np.uint8)
    pad[:n] = inl
    return np.packbits(pad.reshape(words, 64), axis=1, bitorder="little").view("<u8").reshape(words)


def unpack_bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")[:n].astype(bool)


def table(job):
    """every hypothesis of job["samples"] -> (n_inliers[n_hyp] int32, srt[n_hyp][13] float32, bits[n_hyp][words] uint64)"""
    sm = np.asarray(job["samples"], np.int32).reshape(-1, 3)
    n = len(job["X1"])
    ni = np.zeros(len(sm), np.int32)
    srt = np.zeros((len(sm), 13), f)
    bits = np.zeros((len(sm), (n + 63) // 64), np.uint64)
    for k, s in enumerate(sm):
        c, v, inl = hypothesis(job, [int(i) for i in s])
        ni[k], srt[k], bits[k] = c, v, pack_bits(inl)
    return ni, srt, bits


def T12_of(srt):
    """mT12i = [ms12i * mR12i | mt12i; 0 0 0 1] from a table row (:328-333)"""
    T = np.eye(4, dtype=f)
    with np.errstate(all="ignore"):
        T[:3, :3] = (d(srt[0]) * srt[1:10].astype(d)).astype(f).reshape(3, 3)
    T[:3, 3] = srt[10:13]
    return T


def ransac_iterations(probability, min_inliers, max_iterations, N):
    """SetRansacParameters (:117-141) -> mRansacMaxIts"""
    if min_inliers == N:
        n_it = 1
    else:
        with np.errstate(all="ignore"):
            eps = f(min_inliers) / f(N)                     # (float)mRansacMinInliers / N
            x = np.log(d(1.0) - d(probability)) / np.log(d(1.0) - d(math.pow(float(eps), 3.0)) if np.isfinite(eps) else d(np.nan))
        n_it = -2 ** 31 if not np.isfinite(x) else int(math.ceil(float(x)))   # a NaN converts to INT_MIN on the reference's platform
    return max(1, min(n_it, max_iterations))


class _Ransac:
    """the state Sim3Solver keeps between calls; evaluate(k) -> (n_inliers, srt, inliers bool[N]) for the k-th drawn hypothesis"""

    def __init__(self, N, mN1, indices1, probability=0.99, min_inliers=6, max_iterations=300):
        self.N, self.mN1, self.indices1 = N, mN1, np.asarray(indices1, np.int64)
        self.iterations = 0
        self.best_inliers = 0
        self.best = None          # (hypothesis index, srt, inliers)
        self.set_ransac_parameters(probability, min_inliers, max_iterations)

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.min_inliers = min_inliers
        self.max_its = ransac_iterations(probability, min_inliers, max_iterations, self.N)
        self.iterations = 0

    def iterate(self, n_iterations):
        """-> (returned hypothesis index or None, bNoMore, vbInliers[mN1], nInliers)"""
        vb = np.zeros(self.mN1, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            cur += 1
            self.iterations += 1
            k = self.iterations - 1
            ni, srt, inl = self.evaluate(k)
            if ni >= self.best_inliers:
                self.best_inliers = ni
                self.best = (k, srt.copy(), inl.copy())
                if ni > self.min_inliers:
                    vb[self.indices1[inl]] = True
                    return k, False, vb, ni
        return None, self.iterations >= self.max_its, vb, 0

    def find(self):
        k, _, vb, ni = self.iterate(self.max_its)
        return k, vb, ni


class Sequential(_Ransac):
    """the literal loop: hypothesis k is computed when the loop reaches it"""

    def __init__(self, job, mN1=None, indices1=None, **kw):
        self.job = job
        self.evaluated = 0
        n = len(job["X1"])
        super().__init__(n, n if mN1 is None else mN1, np.arange(n) if indices1 is None else indices1, **kw)

    def evaluate(self, k):
        self.evaluated += 1
        return hypothesis(self.job, [int(i) for i in np.asarray(self.job["samples"]).reshape(-1, 3)[k]])


class Replay(_Ransac):
    """the adaptor's form: the whole table first (here handed in), then the same state machine reading rows"""

    def __init__(self, N, tab, mN1=None, indices1=None, **kw):
        self.tab = tab
        super().__init__(N, N if mN1 is None else mN1, np.arange(N) if indices1 is None else indices1, **kw)

    def evaluate(self, k):
        ni, srt, bits = self.tab
        return int(ni[k]), srt[k], unpack_bits(bits[k], self.N)


# ---- the float64 yardstick: the exact Horn formulas with numpy.linalg.eigh on the same float inputs

def horn_f64(P1, P2, fix_scale):
    """-> (s, R[3][3], t[3]) in float64"""
    A, B = np.asarray(P1, d).T, np.asarray(P2, d).T      # [row][point]
    O1, O2 = A.mean(1), B.mean(1)
    Pr1, Pr2 = A - O1[:, None], B - O2[:, None]
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, np.argmax(w)]
    q = q / np.linalg.norm(q)
    a, x, y, z = q
    R = np.array([[a * a + x * x - y * y - z * z, 2 * (x * y - a * z), 2 * (x * z + a * y)],
                  [2 * (x * y + a * z), a * a - x * x + y * y - z * z, 2 * (y * z - a * x)],
                  [2 * (x * z - a * y), 2 * (y * z + a * x), a * a - x * x - y * y + z * z]])
    P3 = R @ Pr2
    s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
    t = O1 - s * (R @ O2)
    return s, R, t, w


def collinearity(P):
    """sin of the smallest angle of the triangle of three points (0: collinear or coincident)"""
    P = np.asarray(P, d)
    best = 1.0
    for i in range(3):
        a, b = P[(i + 1) % 3] - P[i], P[(i + 2) % 3] - P[i]
        na, nb = np.linalg.norm(a), np.linalg.norm(b)
        if na == 0 or nb == 0:
            return 0.0
        best = min(best, float(np.linalg.norm(np.cross(a, b)) / (na * nb)))
    return best
