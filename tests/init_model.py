"""The monocular-initialisation contract of include/orbx.h (orbx_mono_init_hypotheses and what follows it) restated in numpy, one operation
at a time in np.float32 / np.float64, independent of the library: Normalize, the one Jacobi routine behind every SVD of
Initializer.cc, the tables of FindHomography / FindFundamental, the choice, ReconstructH / ReconstructF over CheckRT, and Initialize's
control flow in two formulations (array forms in `initialize`, the reference's sequential text in `sequential`).

Everything that runs once per hypothesis or once per match is written over a leading batch axis: an elementwise numpy operation on
float32 arrays rounds every element once, exactly as the scalar operation does, so batching changes no bit.

A job is a dict(xy1[n1][2], xy2[n2][2], matches[n][2], K[4] = fx fy cx cy, sigma, min_parallax, min_triangulated, samples[n_hyp][8])."""
import math

import numpy as np

F = np.float32
D = np.float64
EPS2 = D(F(2.0) * F(1.1920928955078125e-7))
FLT_MIN = D(1.17549435e-38)
QNAN = np.array([0x7FC00000], np.uint32).view(F)[0]


def _f(a):
    return np.asarray(a, F)


def _d(a):
    return np.asarray(a, F).astype(D)


# ---------------------------------------------------------------------------------------------------------------- small matrices

def mm(X, Y):
    """cv::Mat product over leading batch axes: (float)dotd(X.row(r), Y.col(c)), the sum left to right"""
    X, Y = _d(X), _d(Y)
    out = np.zeros(np.broadcast_shapes(X.shape[:-2], Y.shape[:-2]) + (X.shape[-2], Y.shape[-1]), F)
    assert X.shape[-1] == 3 and Y.shape[-2] == 3
    for r in range(X.shape[-2]):
        for c in range(Y.shape[-1]):
            out[..., r, c] = ((X[..., r, 0] * Y[..., 0, c] + X[..., r, 1] * Y[..., 1, c]) + X[..., r, 2] * Y[..., 2, c]).astype(F)
    return out


def dotd(a, b):
    a, b = _d(a), _d(b)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def det3(M):
    m = _d(M).reshape(M.shape[:-2] + (9,))
    m0, m1, m2, m3, m4, m5, m6, m7, m8 = [m[..., k] for k in range(9)]
    return (m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6)) + m2 * (m3 * m7 - m4 * m6)


def inv3(M):
    """cv::Mat::inv of a 3 x 3: nine zeros where the determinant is zero"""
    M = _f(M)
    m = M.astype(D).reshape(M.shape[:-2] + (9,))
    m0, m1, m2, m3, m4, m5, m6, m7, m8 = [m[..., k] for k in range(9)]
    det = det3(M)
    with np.errstate(all="ignore"):
        d = D(1.0) / det
        cof = [m4 * m8 - m5 * m7, m2 * m7 - m1 * m8, m1 * m5 - m2 * m4,
               m5 * m6 - m3 * m8, m0 * m8 - m2 * m6, m2 * m3 - m0 * m5,
               m3 * m7 - m4 * m6, m1 * m6 - m0 * m7, m0 * m4 - m1 * m3]
        out = np.stack([(c * d).astype(F) for c in cof], -1)
    out = np.where((det == 0)[..., None], F(0.0), out)
    return out.reshape(M.shape).astype(F)


def normalize(xy):
    """Normalize (:831-883) over all keypoints in index order -> (meanX, meanY, sX, sY), T"""
    xy = _f(xy)
    N = F(len(xy))
    meanX = F(0.0); meanY = F(0.0)
    for i in range(len(xy)):
        meanX = meanX + xy[i, 0]; meanY = meanY + xy[i, 1]
    meanX = meanX / N; meanY = meanY / N
    devX = F(0.0); devY = F(0.0)
    for i in range(len(xy)):
        devX = devX + abs(xy[i, 0] - meanX); devY = devY + abs(xy[i, 1] - meanY)
    devX = devX / N; devY = devY / N
    with np.errstate(all="ignore"):
        sX = F(D(1.0) / D(devX)); sY = F(D(1.0) / D(devY))
        T = np.array([[sX, 0, (-meanX) * sX], [0, sY, (-meanY) * sY], [0, 0, 1]], F)
    return np.array([meanX, meanY, sX, sY], F), T


# ---------------------------------------------------------------------------------------------------------------- the Jacobi routine

def _rotation(al, be, g):
    """(rotate, c, s) of one pivot from its three double sums"""
    with np.errstate(all="ignore"):
        rotate = ~(np.abs(g) <= EPS2 * np.sqrt(al * be))
        g2 = g * D(2.0)
        beta = al - be
        gamma = np.sqrt(g2 * g2 + beta * beta)
        neg = beta < 0
        delta = (gamma - beta) * D(0.5)
        s_n = np.sqrt(delta / gamma).astype(F)
        c_n = (g2 / ((gamma * s_n.astype(D)) * D(2.0))).astype(F)
        c_p = np.sqrt((gamma + beta) / (gamma * D(2.0))).astype(F)
        s_p = (g2 / ((gamma * c_p.astype(D)) * D(2.0))).astype(F)
    return rotate, np.where(neg, c_n, c_p), np.where(neg, s_n, s_p)


def _sum16(prod):
    """the stated butterfly of the contract over 16 slots: slot i = 0.0 + the product of row i (0.0 beyond the rows), strides 8, 4, 2, 1"""
    B, m = prod.shape
    assert m <= 16
    v = np.zeros((B, 16), D)
    v[:, :m] = D(0.0) + prod
    lanes = np.arange(16)
    for st in (8, 4, 2, 1):
        v = v + v[:, lanes ^ st]
    return v[:, 0].copy()


def jacobi(A):
    """"SVD" of the contract on A[batch][m][n], n odd -> (the rotated A, V[batch][n][n], W2[batch][n])"""
    A = _f(A).copy()
    B, m, n = A.shape
    assert n % 2 == 1
    V = np.zeros((B, n, n), F)
    V[:, range(n), range(n)] = F(1.0)
    for _sweep in range(30):
        changed = np.zeros(B, bool)
        for r in range(n):
            for k in range(1, (n - 1) // 2 + 1):
                a, b = (r + k) % n, (r - k) % n
                p, q = min(a, b), max(a, b)
                x, y = A[:, :, p].astype(D), A[:, :, q].astype(D)
                al, be, g = _sum16(x * x), _sum16(y * y), _sum16(x * y)
                rotate, c, s = _rotation(al, be, g)
                if not rotate.any():
                    continue
                changed |= rotate
                with np.errstate(all="ignore"):
                    for Mx in (A, V):
                        X, Y = Mx[:, :, p].copy(), Mx[:, :, q].copy()
                        t0 = c[:, None] * X + s[:, None] * Y
                        t1 = (-s)[:, None] * X + c[:, None] * Y
                        Mx[:, :, p] = np.where(rotate[:, None], t0, X)
                        Mx[:, :, q] = np.where(rotate[:, None], t1, Y)
        if not changed.any():
            break
    W2 = np.zeros((B, n), D)
    Ad = A.astype(D)
    with np.errstate(all="ignore"):
        for i in range(m):
            W2 = W2 + Ad[:, i, :] * Ad[:, i, :]
    return A, V, W2


def null_of(A):
    """"null": column j of V for the smallest W2[j], of equal ones the later -> [batch][n]"""
    _, V, W2 = jacobi(A)
    B, n = W2.shape
    col = np.zeros(B, int)
    best = W2[:, 0].copy()
    for j in range(1, n):
        take = W2[:, j] <= best
        best = np.where(take, W2[:, j], best)
        col = np.where(take, j, col)
    return V[np.arange(B), :, col], col


def usv3(M):
    """"U w Vt" of the contract on M[batch][3][3] -> U, w[batch][3], Vt"""
    A, V, W2 = jacobi(M)
    B = len(A)
    U = np.zeros((B, 3, 3), F); w = np.zeros((B, 3), F); Vt = np.zeros((B, 3, 3), F)
    for bi in range(B):
        used = []
        for r in range(3):
            best = -1
            for j in range(3):
                if j in used:
                    continue
                if best < 0 or W2[bi, j] > W2[bi, best]:
                    best = j
            used.append(best)
            with np.errstate(all="ignore"):
                wd = np.sqrt(W2[bi, best])
                sc = F(D(1.0) / wd) if wd > FLT_MIN else F(0.0)
                w[bi, r] = F(wd)
                U[bi, :, r] = A[bi, :, best] * sc
            Vt[bi, r, :] = V[bi, :, best]
    return U, w, Vt


# ---------------------------------------------------------------------------------------------------------------- the table

def gather(job):
    """(u1, v1, u2, v2) per match"""
    xy1, xy2, ma = _f(job["xy1"]), _f(job["xy2"]), np.asarray(job["matches"], int)
    return np.concatenate([xy1[ma[:, 0]], xy2[ma[:, 1]]], 1)


def sample_points(job):
    """the normalised (u1, v1, u2, v2) of every sample row [n_hyp][8][4], T1, T2"""
    n1_, T1 = normalize(job["xy1"])
    n2_, T2 = normalize(job["xy2"])
    pts = gather(job)[np.asarray(job["samples"], int)]
    with np.errstate(all="ignore"):
        u1 = (pts[..., 0] - n1_[0]) * n1_[2]; v1 = (pts[..., 1] - n1_[1]) * n1_[3]
        u2 = (pts[..., 2] - n2_[0]) * n2_[2]; v2 = (pts[..., 3] - n2_[1]) * n2_[3]
    return np.stack([u1, v1, u2, v2], -1).astype(F), T1, T2


def system_h(sp):
    """A of ComputeH21 (:274-301) [n_hyp][16][9]"""
    u1, v1, u2, v2 = [sp[..., k] for k in range(4)]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    with np.errstate(all="ignore"):
        r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
        r1 = np.stack([u1, v1, o, z, z, z, (-u2) * u1, (-u2) * v1, -u2], -1)
    return np.stack([r0, r1], 2).reshape(len(sp), 16, 9).astype(F)


def system_f(sp):
    """A of ComputeF21 (:329-345) [n_hyp][8][9]"""
    u1, v1, u2, v2 = [sp[..., k] for k in range(4)]
    with np.errstate(all="ignore"):
        return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(F)


def models(job):
    """H21i, H12i, F21i of every sample row"""
    sp, T1, T2 = sample_points(job)
    Hn = null_of(system_h(sp))[0].reshape(-1, 3, 3)
    H21 = mm(mm(inv3(T2), Hn), T1)
    H12 = inv3(H21)
    Fpre = null_of(system_f(sp))[0].reshape(-1, 3, 3)
    U, w, Vt = usv3(Fpre)
    Dg = np.zeros_like(U)
    Dg[:, 0, 0] = w[:, 0]; Dg[:, 1, 1] = w[:, 1]
    Fn = mm(mm(U, Dg), Vt)
    F21 = mm(mm(T2.T.copy(), Fn), T1)
    return H21, H12, F21


def _chi_h(H21, H12, pts, inv_s2):
    u1, v1, u2, v2 = [pts[None, :, k] for k in range(4)]
    h = H21.reshape(-1, 9)[:, :, None]; hi = H12.reshape(-1, 9)[:, :, None]
    w2 = (D(1.0) / (hi[:, 6] * u2 + hi[:, 7] * v2 + hi[:, 8]).astype(D)).astype(F)
    u2in1 = (hi[:, 0] * u2 + hi[:, 1] * v2 + hi[:, 2]) * w2
    v2in1 = (hi[:, 3] * u2 + hi[:, 4] * v2 + hi[:, 5]) * w2
    chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2
    w1 = (D(1.0) / (h[:, 6] * u1 + h[:, 7] * v1 + h[:, 8]).astype(D)).astype(F)
    u1in2 = (h[:, 0] * u1 + h[:, 1] * v1 + h[:, 2]) * w1
    v1in2 = (h[:, 3] * u1 + h[:, 4] * v1 + h[:, 5]) * w1
    chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2
    return chi1, chi2


def _chi_f(F21, pts, inv_s2):
    u1, v1, u2, v2 = [pts[None, :, k] for k in range(4)]
    f = F21.reshape(-1, 9)[:, :, None]
    a2 = f[:, 0] * u1 + f[:, 1] * v1 + f[:, 2]
    b2 = f[:, 3] * u1 + f[:, 4] * v1 + f[:, 5]
    c2 = f[:, 6] * u1 + f[:, 7] * v1 + f[:, 8]
    num2 = a2 * u2 + b2 * v2 + c2
    chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
    a1 = f[:, 0] * u2 + f[:, 3] * v2 + f[:, 6]
    b1 = f[:, 1] * u2 + f[:, 4] * v2 + f[:, 7]
    c1 = f[:, 2] * u2 + f[:, 5] * v2 + f[:, 8]
    num1 = a1 * u1 + b1 * v1 + c1
    chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
    return chi1, chi2


def _score_and_bits(chi1, chi2, th, th_score):
    """"check" and "score": the gates, each lane's serial sum over i = l (mod 64), the xor butterfly; the mask words"""
    B, n = chi1.shape
    words = (n + 63) // 64
    acc = np.zeros((B, 64), F)
    bits = np.zeros((B, words), np.uint64)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for wd in range(words):
            m = min(64, n - 64 * wd)
            inl = np.zeros((B, 64), bool)
            inl[:, :m] = True
            for chi in (chi1, chi2):
                c = np.zeros((B, 64), F)
                c[:, :m] = chi[:, 64 * wd:64 * wd + m]
                out = c > th
                valid = np.zeros((B, 64), bool)
                valid[:, :m] = True
                acc = np.where(valid & ~out, acc + (th_score - c), acc)
                inl &= ~out
            bits[:, wd] = (inl.astype(np.uint64) << lanes.astype(np.uint64)[None, :]).sum(1, dtype=np.uint64)
        for s in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ s]
    return acc[:, 0].copy(), bits


def inv_sigma2(sigma):
    s = F(sigma)
    return F(D(1.0) / D(s * s))


def canon(a):
    """every NaN as the quiet NaN 0x7fc00000, the form the contract returns ("NaN")"""
    a = np.array(a, F)
    a[np.isnan(a)] = QNAN
    return a


def table(job):
    """-> (score_h[n_hyp], H21[n_hyp][9], bits_h[n_hyp][words], score_f, F21, bits_f), as orbx_mono_init_hypotheses returns it"""
    H21, H12, F21 = models(job)
    pts = gather(job)
    is2 = inv_sigma2(job.get("sigma", 1.0))
    with np.errstate(all="ignore"):
        sh, bh = _score_and_bits(*_chi_h(H21, H12, pts, is2), F(5.991), F(5.991))
        sf, bf = _score_and_bits(*_chi_f(F21, pts, is2), F(3.841), F(5.991))
    return canon(sh), canon(H21.reshape(-1, 9)), bh, canon(sf), canon(F21.reshape(-1, 9)), bf


def mask_bools(bits, n):
    """mask words -> bool[n]"""
    bits = np.asarray(bits, np.uint64).reshape(-1)
    return np.array([(int(bits[i >> 6]) >> (i & 63)) & 1 for i in range(n)], bool)


def mask_words(flags):
    """bool[n] -> mask words"""
    flags = np.asarray(flags, bool)
    out = np.zeros((len(flags) + 63) // 64, np.uint64)
    for i in np.nonzero(flags)[0]:
        out[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return out


# ---------------------------------------------------------------------------------------------------------------- choice, motions

def best_of(scores):
    """"choice": the earliest strictly greatest score above 0 -> (index or -1, its score or 0)"""
    s = np.where(np.isnan(scores), F(-1.0), scores)
    if len(s) == 0 or not (s.max() > 0):
        return -1, F(0.0)
    k = int(np.argmax(s))   # numpy's argmax returns the first of equal maxima
    return k, F(scores[k])


def choose(tab):
    bh, SH = best_of(tab[0])
    bf, SF = best_of(tab[3])
    with np.errstate(all="ignore"):
        RH = F(SH) / (F(SH) + F(SF))
    takeH = bool(D(RH) > D(0.40))
    best = bh if takeH else bf
    model = 0 if best < 0 else (1 if takeH else 2)
    return dict(model=model, best_h=bh, best_f=bf, SH=SH, SF=SF)


def kmat(K):
    fx, fy, cx, cy = _f(K)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)


def _normalised(t):
    with np.errstate(all="ignore"):
        inv = D(1.0) / np.sqrt(dotd(t, t))
        return (_d(t) * inv).astype(F)


def fsqrt(x):
    with np.errstate(all="ignore"):
        return F(np.sqrt(D(F(x))))


def motions(model, M, K):
    """the rows of ReconstructH (8) / ReconstructF (4) -> [(R, t)], or None for ReconstructH's early return"""
    Km = kmat(K)
    M = _f(M).reshape(3, 3)
    with np.errstate(all="ignore"):
        if model == 1:
            A = mm(mm(inv3(Km), M), Km)
            U, w, Vt = [a[0] for a in usv3(A[None])]
            s = F(det3(U) * det3(Vt))
            d1, d2, d3 = w
            if D(d1 / d2) < D(1.00001) or D(d2 / d3) < D(1.00001):
                return None
            aux1 = fsqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
            aux3 = fsqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
            x1 = [aux1, aux1, -aux1, -aux1]
            x3 = [aux3, -aux3, aux3, -aux3]
            aux_st = fsqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
            ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
            st = [aux_st, -aux_st, -aux_st, aux_st]
            aux_sp = fsqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
            cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
            sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
            sU = (s * U).astype(F)
            rows = []
            for i in range(8):
                j = i & 3
                if i < 4:
                    Rp = np.array([[ct, 0, -st[j]], [0, 1, 0], [st[j], 0, ct]], F)
                    tp = np.array([x1[j] * (d1 - d3), F(0.0) * (d1 - d3), (-x3[j]) * (d1 - d3)], F)
                else:
                    Rp = np.array([[cp, 0, sp[j]], [0, -1, 0], [sp[j], 0, -cp]], F)
                    tp = np.array([x1[j] * (d1 + d3), F(0.0) * (d1 + d3), x3[j] * (d1 + d3)], F)
                R = mm(mm(sU, Rp), Vt)
                t = np.array([F(dotd(U[r], tp)) for r in range(3)], F)
                rows.append((R, _normalised(t)))
            return rows
        E = mm(mm(Km.T.copy(), M), Km)
        U, w, Vt = [a[0] for a in usv3(E[None])]
        t = _normalised(U[:, 2].copy())
        W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
        R1 = mm(mm(U, W), Vt)
        if det3(R1) < 0:
            R1 = -R1
        R2 = mm(mm(U, W.T.copy()), Vt)
        if det3(R2) < 0:
            R2 = -R2
        return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


# ---------------------------------------------------------------------------------------------------------------- CheckRT

def null4(A):
    """the 4x4 routine of the triangulation block on A[batch][4][4] (tests/triangulate_model.py: null_vector, here over a batch):
    lexicographic pairs, the squared norms carried along -> v[batch][4]"""
    At = np.transpose(_f(A), (0, 2, 1)).copy()   # At[b][i] = column i
    B = len(At)
    V = np.zeros((B, 4, 4), F)
    V[:, range(4), range(4)] = F(1.0)
    Ad = At.astype(D)
    W = np.zeros((B, 4), D)
    for k in range(4):
        W = W + Ad[:, :, k] * Ad[:, :, k]
    with np.errstate(all="ignore"):
        for _sweep in range(30):
            changed = np.zeros(B, bool)
            for i in range(3):
                for j in range(i + 1, 4):
                    p = np.zeros(B, D)
                    for k in range(4):
                        p = p + At[:, i, k].astype(D) * At[:, j, k].astype(D)
                    rotate, c, s = _rotation(W[:, i], W[:, j], p)
                    if not rotate.any():
                        continue
                    changed |= rotate
                    X, Y = At[:, i].copy(), At[:, j].copy()
                    t0 = c[:, None] * X + s[:, None] * Y
                    t1 = (-s)[:, None] * X + c[:, None] * Y
                    a = np.zeros(B, D); b = np.zeros(B, D)
                    for k in range(4):
                        a = a + t0[:, k].astype(D) * t0[:, k].astype(D)
                        b = b + t1[:, k].astype(D) * t1[:, k].astype(D)
                    At[:, i] = np.where(rotate[:, None], t0, X); At[:, j] = np.where(rotate[:, None], t1, Y)
                    W[:, i] = np.where(rotate, a, W[:, i]); W[:, j] = np.where(rotate, b, W[:, j])
                    X, Y = V[:, i].copy(), V[:, j].copy()
                    V[:, i] = np.where(rotate[:, None], c[:, None] * X + s[:, None] * Y, X)
                    V[:, j] = np.where(rotate[:, None], (-s)[:, None] * X + c[:, None] * Y, Y)
            if not changed.any():
                break
        Ad = At.astype(D)
        sd = np.zeros((B, 4), D)
        for k in range(4):
            sd = sd + Ad[:, :, k] * Ad[:, :, k]
    sel = np.zeros(B, int)
    best = sd[:, 0].copy()
    for i in range(1, 4):
        take = sd[:, i] <= best
        best = np.where(take, sd[:, i], best); sel = np.where(take, i, sel)
    return V[np.arange(B), sel]


def cos_key(c):
    """an unsigned key in the order of the floats, every NaN above every number"""
    b = np.asarray(c, F).view(np.uint32).astype(np.uint64)
    k = np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    return np.where(np.isnan(c), 0xFFFFFFFE, k).astype(np.uint32)


def key_cos(k):
    k = int(k)
    if k == 0xFFFFFFFE:
        return QNAN
    b = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(F)[0]


def th2_of(sigma):
    s = F(sigma)
    return F(D(4.0) * D(s * s))


def check_rt(job, R, t, inl):
    """CheckRT (:886-1004) for the matches inl[n] -> (n_good, the ranked cosine, p3d[n][3], flag[n]: 0 / 1 accepted / 2 with parallax)"""
    fx, fy, cx, cy = _f(job["K"])
    Km = kmat(job["K"])
    pts = gather(job)
    n = len(pts)
    th2 = th2_of(job.get("sigma", 1.0))
    R, t = _f(R), _f(t)
    Rt = np.concatenate([R, t[:, None]], 1)
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], F)
    P2 = mm(Km, Rt)
    O2 = np.array([F(-dotd(R[:, r], t)) for r in range(3)], F)
    idx = np.nonzero(np.asarray(inl, bool))[0]
    p3d = np.zeros((n, 3), F); flag = np.zeros(n, np.uint8)
    if len(idx) == 0:
        return 0, F(1.0), p3d, flag
    u1, v1, u2, v2 = [pts[idx, k] for k in range(4)]
    with np.errstate(all="ignore"):
        A = np.stack([u1[:, None] * P1[2][None] - P1[0][None], v1[:, None] * P1[2][None] - P1[1][None],
                      u2[:, None] * P2[2][None] - P2[0][None], v2[:, None] * P2[2][None] - P2[1][None]], 1).astype(F)
        v = null4(A)
        p = (v[:, :3] / v[:, 3:4]).astype(F)
        ok = np.isfinite(p).all(1)
        dist1 = np.sqrt(dotd(p, p)).astype(F)
        n2 = (p - O2[None]).astype(F)
        dist2 = np.sqrt(dotd(n2, n2)).astype(F)
        cosp = (dotd(p, n2) / (dist1 * dist2).astype(D)).astype(F)
        low = cosp.astype(D) < D(0.99998)
        ok &= ~((p[:, 2] <= 0) & low)
        q = np.stack([(dotd(R[r][None], p) + D(t[r])).astype(F) for r in range(3)], 1)
        ok &= ~((q[:, 2] <= 0) & low)
        invZ1 = (D(1.0) / p[:, 2].astype(D)).astype(F)
        im1x = fx * p[:, 0] * invZ1 + cx; im1y = fy * p[:, 1] * invZ1 + cy
        ok &= ~((im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1) > th2)
        invZ2 = (D(1.0) / q[:, 2].astype(D)).astype(F)
        im2x = fx * q[:, 0] * invZ2 + cx; im2y = fy * q[:, 1] * invZ2 + cy
        ok &= ~((im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2) > th2)
    p3d[idx[ok]] = p[ok]
    flag[idx[ok]] = np.where(low[ok], 2, 1)
    n_good = int(ok.sum())
    if n_good == 0:
        return 0, F(1.0), p3d, flag
    keys = np.sort(cos_key(cosp[ok]))
    return n_good, key_cos(keys[min(50, n_good - 1)]), p3d, flag


# ---------------------------------------------------------------------------------------------------------------- acos

def degrees(c):
    """(float)(acos((double)c) * 180 / CV_PI) through the C library"""
    c = float(F(c))
    a = math.acos(c) if -1.0 <= c <= 1.0 else float("nan")
    return canon(F(a * 180 / 3.1415926535897932384626433832795))[()]


def _unkey(k):
    return key_cos(k)


def cos_threshold(min_parallax, ge):
    """"acos": the smallest float of [-1, 1] whose parallax fails `>= min_parallax` (ge) or `> min_parallax`; the float above 1 if none"""
    mp = F(min_parallax)

    def passes(k):
        d = degrees(_unkey(k))
        return bool(d >= mp) if ge else bool(d > mp)
    lo, hi = int(cos_key(F(-1.0))), int(cos_key(F(1.0))) + 1
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if passes(mid):
            lo = mid + 1
        else:
            hi = mid
    return _unkey(lo)


def parallax_passes(c, thr):
    return bool(c >= F(-1.0)) and bool(c < thr)


# ---------------------------------------------------------------------------------------------------------------- reconstruction

def _empty_recon(n1):
    return dict(ok=False, winner=-1, n_good=np.zeros(8, np.int32), cos_parallax=np.ones(8, F), R=np.zeros((8, 3, 3), F), t=np.zeros((8, 3), F),
                P3D=np.zeros((n1, 3), F), triangulated=np.zeros(n1, bool))


def reconstruct(job, model, M, mask):
    """orbx_mono_init_reconstruct -> dict(ok, winner, n_good[8], cos_parallax[8], R[8][3][3], t[8][3], P3D[n1][3], triangulated[n1])"""
    n1, n = len(job["xy1"]), len(job["matches"])
    out = _empty_recon(n1)
    rows = motions(model, M, job["K"])
    if rows is None:
        return out
    inl = mask_bools(mask, n)
    N = int(inl.sum())
    pts = []
    for i, (R, t) in enumerate(rows):
        g, c, p3d, flag = check_rt(job, R, t, inl)
        out["n_good"][i] = g; out["cos_parallax"][i] = c; out["R"][i] = canon(R); out["t"][i] = canon(t)
        pts.append((p3d, flag))
    mp, mt = job.get("min_parallax", 1.0), int(job.get("min_triangulated", 50))
    good = out["n_good"]
    ok, winner = False, -1
    if model == 1:   # "decide H" in array form: the first maximum is the best, the second is the largest of the others
        if good.max() > 0:
            winner = int(np.argmax(good))
            second = int(np.delete(good, winner).max())
            best = int(good[winner])
            ok = (D(second) < D(0.75) * D(best) and parallax_passes(out["cos_parallax"][winner], cos_threshold(mp, True))
                  and best > mt and D(best) > D(0.9) * D(N))
    else:
        g4 = good[:4]
        maxg = int(g4.max())
        nmin = max(int(D(0.9) * D(N)), mt)
        nsim = int((g4.astype(D) > D(0.7) * D(maxg)).sum())
        if not (maxg < nmin or nsim > 1):
            winner = int(np.argmax(g4))
            ok = parallax_passes(out["cos_parallax"][winner], cos_threshold(mp, False))
    out["ok"], out["winner"] = bool(ok), winner
    if ok:
        p3d, flag = pts[winner]
        first = np.asarray(job["matches"], int)[:, 0]
        acc = flag > 0
        out["P3D"][first[acc]] = p3d[acc]
        out["triangulated"][first[acc]] = flag[acc] == 2
    return out


def initialize(job, tab=None):
    """orbx_mono_init_initialize -> dict(ok, model, best_h, best_f, SH, SF, M[9], R21, t21, parallax, winner, n_good, cos_parallax, P3D,
    triangulated)"""
    tab = table(job) if tab is None else tab
    ch = choose(tab)
    n1 = len(job["xy1"])
    if ch["model"] == 0:
        rec, M = _empty_recon(n1), np.zeros(9, F)
    else:
        M = (tab[1][ch["best_h"]] if ch["model"] == 1 else tab[4][ch["best_f"]]).copy()
        mask = tab[2][ch["best_h"]] if ch["model"] == 1 else tab[5][ch["best_f"]]
        rec = reconstruct(job, ch["model"], M, mask)
    w = rec["winner"]
    out = dict(ch, M=M, R21=np.zeros((3, 3), F), t21=np.zeros(3, F), parallax=degrees(rec["cos_parallax"][w]) if w >= 0 else F(0.0))
    out.update(ok=rec["ok"], winner=w, n_good=rec["n_good"], cos_parallax=rec["cos_parallax"], P3D=rec["P3D"], triangulated=rec["triangulated"])
    if rec["ok"]:
        out["R21"], out["t21"] = rec["R"][w].copy(), rec["t"][w].copy()
    return out


def sequential(job, tab):
    """Initialize's control flow as the reference writes it (:179-209, :240-263, :133-142, :569-639, :769-811), one statement after the
    other over the rows of the table; parallax in DEGREES through acos, as the text has it -> (ok, model, R21, t21, P3D, triangulated)"""
    n1, n = len(job["xy1"]), len(job["matches"])
    mp, mt = F(job.get("min_parallax", 1.0)), int(job.get("min_triangulated", 50))
    score, best = F(0.0), -1
    for it in range(len(tab[0])):
        if tab[0][it] > score:
            score, best = tab[0][it], it
    SH, bh = score, best
    score, best = F(0.0), -1
    for it in range(len(tab[3])):
        if tab[3][it] > score:
            score, best = tab[3][it], it
    SF, bf = score, best
    with np.errstate(all="ignore"):
        RH = SH / (SH + SF)
    fail = (False, 0, None, None, np.zeros((n1, 3), F), np.zeros(n1, bool))
    first = np.asarray(job["matches"], int)[:, 0]

    def run(R, t, inl):
        g, c, p3d, flag = check_rt(job, R, t, inl)
        P = np.zeros((n1, 3), F); tri = np.zeros(n1, bool)
        P[first[flag > 0]] = p3d[flag > 0]; tri[first[flag > 0]] = flag[flag > 0] == 2
        return g, (degrees(c) if g > 0 else F(0.0)), P, tri

    if D(RH) > 0.40:
        if bh < 0:
            return fail
        inl = mask_bools(tab[2][bh], n)
        N = int(inl.sum())
        rows = motions(1, tab[1][bh], job["K"])
        if rows is None:
            return (False, 1) + fail[2:]
        bestGood, secondBestGood, bestIdx, bestParallax, bestP, bestT = 0, 0, -1, F(-1.0), None, None
        for i in range(8):
            nGood, par, P, tri = run(rows[i][0], rows[i][1], inl)
            if nGood > bestGood:
                secondBestGood = bestGood; bestGood = nGood; bestIdx = i; bestParallax = par; bestP, bestT = P, tri
            elif nGood > secondBestGood:
                secondBestGood = nGood
        if secondBestGood < 0.75 * bestGood and bestParallax >= mp and bestGood > mt and bestGood > 0.9 * N:
            return True, 1, rows[bestIdx][0], rows[bestIdx][1], bestP, bestT
        return (False, 1) + fail[2:]
    if bf < 0:
        return fail
    inl = mask_bools(tab[5][bf], n)
    N = int(inl.sum())
    rows = motions(2, tab[4][bf], job["K"])
    res = [run(R, t, inl) for R, t in rows]
    nGood1, nGood2, nGood3, nGood4 = [r[0] for r in res]
    maxGood = max(nGood1, max(nGood2, max(nGood3, nGood4)))
    nMinGood = max(int(0.9 * N), mt)
    nsimilar = 0
    if nGood1 > 0.7 * maxGood:
        nsimilar += 1
    if nGood2 > 0.7 * maxGood:
        nsimilar += 1
    if nGood3 > 0.7 * maxGood:
        nsimilar += 1
    if nGood4 > 0.7 * maxGood:
        nsimilar += 1
    if maxGood < nMinGood or nsimilar > 1:
        return (False, 2) + fail[2:]
    if maxGood == nGood1:
        k = 0
    elif maxGood == nGood2:
        k = 1
    elif maxGood == nGood3:
        k = 2
    else:
        k = 3
    if res[k][1] > mp:
        return True, 2, rows[k][0], rows[k][1], res[k][2], res[k][3]
    return (False, 2) + fail[2:]
