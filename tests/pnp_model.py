"""The PnPsolver contract of include/orbx.h (orbx_pnp_hypotheses) restated in numpy, one operation at a time: np.float64 scalars where the
order matters (the sums over correspondences, the Jacobi SVD's dot products, qr_solve) and element-wise arrays where every element is on its
own (the disjoint pivots of a round-robin round, the rows of a rotation, the per-correspondence terms, CheckInliers).  numpy rounds every
element-wise operation on its own and never fuses.  It also holds PnPsolver::iterate (reference src/PnPsolver.cc:176-269) twice:
`Sequential` is the literal loop, which evaluates a hypothesis when it reaches it and refines from the best set so far, as the reference
does; `Replay` walks a finished table whose rows were each refined from their OWN mask."""
import math

import numpy as np

f = np.float32
d = np.float64
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]
SWEEPS = 30
EPS = d(2.0 ** -49)
CUT = d(2.0 ** -51)
ZERO, ONE, TWO, HALF = d(0.0), d(1.0), d(2.0), d(0.5)
LANES = np.arange(64)


# ---- sums over the members

class Members:
    """the correspondences compute_pose runs on: idx in the order of the contract; serial: the four of a sample row"""

    def __init__(self, job, idx, serial):
        self.idx = np.asarray(idx, np.int64)
        self.serial = serial
        self.n = len(job["P3Dw"])
        self.pw = np.asarray(job["P3Dw"], f)[self.idx].astype(d)      # [cnt][3]
        self.uv = np.asarray(job["P2D"], f)[self.idx].astype(d)       # [cnt][2]
        self.nc = d(len(self.idx))

    def sum(self, *terms):
        """SUM of the contract: every term is an array over the members (any trailing shape); a member adds its terms in turn"""
        terms = [np.asarray(t, d) for t in terms]
        shape = terms[0].shape[1:]
        if self.serial:
            acc = np.zeros(shape, d)
            for k in range(len(self.idx)):
                for t in terms:
                    acc = acc + t[k]
            return acc
        words = (self.n + 63) // 64
        full = []
        for t in terms:
            a = np.zeros((words * 64,) + shape, d)
            a[self.idx] = t                  # a non-member adds nothing: acc + 0.0 has acc's bits (acc is never -0.0)
            full.append(a.reshape((words, 64) + shape))
        acc = np.zeros((64,) + shape, d)
        for wd in range(words):
            for a in full:
                acc = acc + a[wd]
        for s in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[LANES ^ s]
        return acc[0]


# ---- the one SVD routine

def round_robin(n):
    """the rounds of a sweep: lists of pivots (p, q), p < q < n"""
    N = (n + 1) & ~1
    out = []
    for r in range(N - 1):
        rnd = []
        for k in range(N // 2):
            a, b = (N - 1, r) if k == 0 else ((r + k) % (N - 1), (r + (N - 1) - k) % (N - 1))
            p, q = min(a, b), max(a, b)
            if q < n:
                rnd.append((p, q))
        out.append(rnd)
    return out


def svd(A, info=None):
    """A: m x n -> (A rotated, V, w).  The pivots of a round are evaluated side by side, element-wise; their dot products serially."""
    with np.errstate(all="ignore"):
        return _svd(A, info)


def _svd(A, info):
    A = np.array(A, d)
    m, n = A.shape
    B = np.concatenate([A, np.eye(n, dtype=d)], 0)
    rounds = [(np.array([p for p, _ in r]), np.array([q for _, q in r])) for r in round_robin(n)]
    sweeps = 0
    for _ in range(SWEEPS):
        changed = False
        sweeps += 1
        for ps, qs in rounds:
            X, Y = B[:m, ps], B[:m, qs]
            al, be, g = np.zeros(len(ps), d), np.zeros(len(ps), d), np.zeros(len(ps), d)
            for i in range(m):
                al = al + X[i] * X[i]
                be = be + Y[i] * Y[i]
                g = g + X[i] * Y[i]
            rot = ~(np.abs(g) <= EPS * np.sqrt(al * be))
            if not rot.any():
                continue
            changed = True
            g2 = g * TWO
            beta = al - be
            gamma = np.sqrt(g2 * g2 + beta * beta)
            delta = (gamma - beta) * HALF
            s_neg = np.sqrt(delta / gamma)
            c_neg = g2 / ((gamma * s_neg) * TWO)
            c_pos = np.sqrt((gamma + beta) / (gamma * TWO))
            s_pos = g2 / ((gamma * c_pos) * TWO)
            neg = beta < ZERO
            c, s = np.where(neg, c_neg, c_pos), np.where(neg, s_neg, s_pos)
            X, Y = B[:, ps], B[:, qs]
            B[:, ps] = np.where(rot, c * X + s * Y, X)
            B[:, qs] = np.where(rot, c * Y - s * X, Y)
        if not changed:
            break
    w = np.zeros(n, d)
    for i in range(m):
        w = w + B[i] * B[i]
    w = np.sqrt(w)
    if info is not None:
        info.setdefault("sweeps", []).append(sweeps)
    return B[:m].copy(), B[m:].copy(), w


def sort_desc(w):
    """descending, of equal values the earlier index first (the selection of the contract)"""
    n = len(w)
    used, order = [False] * n, []
    for _ in range(n):
        best = -1
        for j in range(n):
            if used[j]:
                continue
            if best < 0 or w[j] > w[best]:
                best = j
        order.append(best)
        used[best] = True
    return order


def solve(Ar, V, w, b):
    """x = V diag(1 / w) U^T b behind svd()"""
    m, n = Ar.shape
    total = ZERO
    for k in range(n):
        total = total + w[k]
    thr = total * CUT
    x = [ZERO] * n
    for k in range(n):
        if not (w[k] > thr):
            continue
        t = ZERO
        for i in range(m):
            t = t + Ar[i][k] * b[i]
        t = (t / w[k]) / w[k]
        for j in range(n):
            x[j] = x[j] + V[j][k] * t
    return x


# ---- the reference's own scalar code

def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def qr_solve(A, b, x):
    """:871-961 on lists of np.float64; x is updated in place unless a pivot column is zero"""
    nr, nc = 6, 4
    A1, A2 = [ZERO] * nc, [ZERO] * nc
    for k in range(nc):
        eta = abs(A[k][k])
        for i in range(k, nr - 1):                     # the scan never looks at the last row
            elt = abs(A[i][k])
            if eta < elt:
                eta = elt
        if eta == ZERO:
            return
        inv_eta = ONE / eta
        total = ZERO
        for i in range(k, nr):
            A[i][k] = A[i][k] * inv_eta
            total = total + A[i][k] * A[i][k]
        sigma = np.sqrt(total)
        if A[k][k] < ZERO:
            sigma = -sigma
        A[k][k] = A[k][k] + sigma
        A1[k] = sigma * A[k][k]
        A2[k] = (-eta) * sigma
        for j in range(k + 1, nc):
            sm = ZERO
            for i in range(k, nr):
                sm = sm + A[i][k] * A[i][j]
            tau = sm / A1[k]
            for i in range(k, nr):
                A[i][j] = A[i][j] - tau * A[i][k]
    for j in range(nc):
        tau = ZERO
        for i in range(j, nr):
            tau = tau + A[i][j] * b[i]
        tau = tau / A1[j]
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i][j]
    x[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        total = ZERO
        for j in range(i + 1, nc):
            total = total + A[i][j] * x[j]
        x[i] = (b[i] - total) / A2[i]


def gauss_newton(L, rho, betas):
    x = [ZERO] * 4                                     # defined: the reference reads it uninitialised
    for _ in range(5):
        b0, b1, b2, b3 = betas
        A, bb = [], []
        for i in range(6):
            l = L[i]
            A.append([(((TWO * l[0]) * b0 + l[1] * b1) + l[3] * b2) + l[6] * b3,
                      ((l[1] * b0 + (TWO * l[2]) * b1) + l[4] * b2) + l[7] * b3,
                      ((l[3] * b0 + l[4] * b1) + (TWO * l[5]) * b2) + l[8] * b3,
                      ((l[6] * b0 + l[7] * b1) + l[8] * b2) + (TWO * l[9]) * b3])
            bb.append(rho[i] - ((((((((((l[0] * b0) * b0 + (l[1] * b0) * b1) + (l[2] * b1) * b1) + (l[3] * b0) * b2) + (l[4] * b1) * b2)
                                     + (l[5] * b2) * b2) + (l[6] * b0) * b3) + (l[7] * b1) * b3) + (l[8] * b2) * b3) + (l[9] * b3) * b3))
        qr_solve(A, bb, x)
        betas = [betas[i] + x[i] for i in range(4)]
    return betas


def find_betas(ap, bs):
    """find_betas_approx_1 / _2 / _3 behind the solve (:694-704, :725-736, :759-768)"""
    if ap == 0:
        if bs[0] < ZERO:
            b0 = np.sqrt(-bs[0])
            return [b0, (-bs[1]) / b0, (-bs[2]) / b0, (-bs[3]) / b0]
        b0 = np.sqrt(bs[0])
        return [b0, bs[1] / b0, bs[2] / b0, bs[3] / b0]
    if bs[0] < ZERO:
        b0 = np.sqrt(-bs[0])
        b1 = np.sqrt(-bs[2]) if bs[2] < ZERO else ZERO
    else:
        b0 = np.sqrt(bs[0])
        b1 = np.sqrt(bs[2]) if bs[2] > ZERO else ZERO
    if bs[1] < ZERO:
        b0 = -b0
    return [b0, b1, bs[3] / b0 if ap == 2 else ZERO, ZERO]


COLS = ((0, 1, 3, 6), (0, 1, 2), (0, 1, 2, 3, 4))
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def compute_pose(job, M, info=None, linalg=None):
    """compute_pose (:488-536) on the members M -> (R[3][3], t[3]) float64.  linalg: the independent evaluation -- an object with eig(S)
    -> (w sorted descending, rows = vectors), inv(A), lstsq(A, b), uv(A) -> (U, V) -- in place of the Jacobi restatements."""
    fu, fv, uc, vc = [d(v) for v in np.asarray(job["K"], d)]
    with np.errstate(all="ignore"):
        pw, uv, nc = M.pw, M.uv, M.nc
        # choose_control_points
        c0 = M.sum(pw) / nc
        dw = pw - c0
        ptp6 = M.sum(np.stack([dw[:, 0] * dw[:, 0], dw[:, 0] * dw[:, 1], dw[:, 0] * dw[:, 2], dw[:, 1] * dw[:, 1], dw[:, 1] * dw[:, 2],
                               dw[:, 2] * dw[:, 2]], 1))
        ptp = np.array([[ptp6[0], ptp6[1], ptp6[2]], [ptp6[1], ptp6[3], ptp6[4]], [ptp6[2], ptp6[4], ptp6[5]]], d)
        if linalg is None:
            _, V, w = svd(ptp, info)
            order = sort_desc(w)
            dc, uct = [w[o] for o in order], [V[:, o] for o in order]
        else:
            dc, uct = linalg.eig(ptp)
        cws = [c0] + [c0 + np.sqrt(dc[i] / nc) * uct[i] for i in range(3)]
        # compute_barycentric_coordinates
        cc = np.array([[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)], d)
        if linalg is None:
            Ar, V, w = svd(cc, info)
            ci = np.zeros((3, 3), d)
            for j in range(3):
                ci[:, j] = solve(Ar, V, w, [ONE if i == j else ZERO for i in range(3)])
        else:
            ci = linalg.inv(cc)
        al = np.zeros((len(pw), 4), d)
        for j in range(3):
            al[:, 1 + j] = (ci[j][0] * dw[:, 0] + ci[j][1] * dw[:, 1]) + ci[j][2] * dw[:, 2]
        al[:, 0] = ((ONE - al[:, 1]) - al[:, 2]) - al[:, 3]
        # fill_M, MtM
        M1, M2 = np.zeros((len(pw), 12), d), np.zeros((len(pw), 12), d)
        for q in range(4):
            M1[:, 3 * q] = al[:, q] * fu
            M1[:, 3 * q + 2] = al[:, q] * (uc - uv[:, 0])
            M2[:, 3 * q + 1] = al[:, q] * fv
            M2[:, 3 * q + 2] = al[:, q] * (vc - uv[:, 1])
        jk = [(j, k) for j in range(12) for k in range(j, 12)]
        up = M.sum(np.stack([M1[:, j] * M1[:, k] for j, k in jk], 1), np.stack([M2[:, j] * M2[:, k] for j, k in jk], 1))
        mtm = np.zeros((12, 12), d)
        for e, (j, k) in enumerate(jk):
            mtm[j][k] = mtm[k][j] = up[e]
        if linalg is None:
            _, V, w = svd(mtm, info)
            order = sort_desc(w)
            vt = [V[:, order[11 - i]] for i in range(4)]
        else:
            _, rows = linalg.eig(mtm)
            vt = [rows[11 - i] for i in range(4)]
        # compute_L_6x10, compute_rho
        L = []
        for a, b in PAIRS:
            dv = [[vt[i][3 * a + k] - vt[i][3 * b + k] for k in range(3)] for i in range(4)]
            L.append([dot3(dv[0], dv[0]), TWO * dot3(dv[0], dv[1]), dot3(dv[1], dv[1]), TWO * dot3(dv[0], dv[2]), TWO * dot3(dv[1], dv[2]),
                      dot3(dv[2], dv[2]), TWO * dot3(dv[0], dv[3]), TWO * dot3(dv[1], dv[3]), TWO * dot3(dv[2], dv[3]), dot3(dv[3], dv[3])])
        rho = []
        for a, b in PAIRS:
            e = [cws[a][k] - cws[b][k] for k in range(3)]
            rho.append((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        best = None
        for ap in range(3):
            sub = np.array([[L[i][c] for c in COLS[ap]] for i in range(6)], d)
            if linalg is None:
                Ar, V, w = svd(sub, info)
                bs = solve(Ar, V, w, rho)
            else:
                bs = list(linalg.lstsq(sub, np.array(rho, d)))
            bs = list(bs) + [ZERO] * (5 - len(bs))
            betas = gauss_newton(L, rho, find_betas(ap, bs))
            # compute_ccs, compute_pcs, solve_for_sign
            ccs = np.zeros((4, 3), d)
            for j in range(4):
                for k in range(3):
                    v = ZERO
                    for i in range(4):
                        v = v + betas[i] * vt[i][3 * j + k]
                    ccs[j][k] = v
            a0 = al[0]
            if ((a0[0] * ccs[0][2] + a0[1] * ccs[1][2]) + a0[2] * ccs[2][2]) + a0[3] * ccs[3][2] < ZERO:
                ccs = -ccs
            pc = np.stack([((al[:, 0] * ccs[0][j] + al[:, 1] * ccs[1][j]) + al[:, 2] * ccs[2][j]) + al[:, 3] * ccs[3][j] for j in range(3)], 1)
            # estimate_R_and_t
            pc0 = M.sum(pc) / nc
            dp = pc - pc0
            abt = M.sum(np.stack([dp[:, j] * dw[:, c] for j in range(3) for c in range(3)], 1)).reshape(3, 3)
            if linalg is None:
                Ar, V, w = svd(abt, info)
                U = Ar / w
            else:
                U, V = linalg.uv(abt)
            R = np.array([[dot3(U[i], V[j]) for j in range(3)] for i in range(3)], d)
            det = (((((R[0][0] * R[1][1]) * R[2][2] + (R[0][1] * R[1][2]) * R[2][0]) + (R[0][2] * R[1][0]) * R[2][1])
                    - (R[0][2] * R[1][1]) * R[2][0]) - (R[0][1] * R[1][0]) * R[2][2]) - (R[0][0] * R[1][2]) * R[2][1]
            if det < ZERO:
                R[2] = -R[2]
            t = np.array([pc0[i] - dot3(R[i], c0) for i in range(3)], d)
            # reprojection_error
            Xc = ((R[0][0] * pw[:, 0] + R[0][1] * pw[:, 1]) + R[0][2] * pw[:, 2]) + t[0]
            Yc = ((R[1][0] * pw[:, 0] + R[1][1] * pw[:, 1]) + R[1][2] * pw[:, 2]) + t[1]
            inv_Zc = ONE / (((R[2][0] * pw[:, 0] + R[2][1] * pw[:, 1]) + R[2][2] * pw[:, 2]) + t[2])
            eu, ev = uv[:, 0] - (uc + (fu * Xc) * inv_Zc), uv[:, 1] - (vc + (fv * Yc) * inv_Zc)
            err = M.sum(np.sqrt(eu * eu + ev * ev)) / nc
            if best is None or err < best[0]:
                best = (err, R, t)
            if info is not None:
                info.setdefault("errors", []).append(float(err))
    return best[1], best[2]


def check_inliers(job, R, t):
    """CheckInliers (:319-350) -> bool[n]; a pose that is not finite has none"""
    P, p2 = np.asarray(job["P3Dw"], f).astype(d), np.asarray(job["P2D"], f).astype(d)
    fu, fv, uc, vc = [d(v) for v in np.asarray(job["K"], d)]
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return np.zeros(len(P), bool)
    with np.errstate(all="ignore"):
        Xc = (((R[0][0] * P[:, 0] + R[0][1] * P[:, 1]) + R[0][2] * P[:, 2]) + t[0]).astype(f)
        Yc = (((R[1][0] * P[:, 0] + R[1][1] * P[:, 1]) + R[1][2] * P[:, 2]) + t[1]).astype(f)
        invZc = (ONE / (((R[2][0] * P[:, 0] + R[2][1] * P[:, 1]) + R[2][2] * P[:, 2]) + t[2])).astype(f)
        ue = uc + (fu * Xc.astype(d)) * invZc.astype(d)
        ve = vc + (fv * Yc.astype(d)) * invZc.astype(d)
        dx, dy = (p2[:, 0] - ue).astype(f), (p2[:, 1] - ve).astype(f)
        e2 = dx * dx + dy * dy
        return e2 < np.asarray(job["max_err"], f)


def _rt(R, t):
    v = np.concatenate([np.asarray(R, d).reshape(9), np.asarray(t, d).reshape(3)])
    return v if np.isfinite(v).all() else np.full(12, QNAN, d)


def hypothesis(job, sample):
    """compute_pose on a sample row + CheckInliers -> (n_inliers, Rt[12], inliers bool[n])"""
    R, t = compute_pose(job, Members(job, sample, True))
    inl = check_inliers(job, R, t)
    return int(inl.sum()), _rt(R, t), inl


def refine(job, mask):
    """Refine (:271-316) from a mask -> (n_refined, Rt[12], inliers bool[n])"""
    R, t = compute_pose(job, Members(job, np.nonzero(mask)[0], False))
    inl = check_inliers(job, R, t)
    return int(inl.sum()), _rt(R, t), inl


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
    """every hypothesis of job["samples"], each qualifying row refined from its own mask ->
    (n_inliers[n_hyp] int32, Rt[n_hyp][12], bits[n_hyp][words] uint64, n_refined, Rt_refined, refined_bits)"""
    sm = np.asarray(job["samples"], np.int32).reshape(-1, 4)
    n, nh = len(job["P3Dw"]), len(sm)
    words = (n + 63) // 64
    ni, rt, bits = np.zeros(nh, np.int32), np.zeros((nh, 12), d), np.zeros((nh, words), np.uint64)
    nr, rtr, rbits = np.full(nh, -1, np.int32), np.full((nh, 12), QNAN, d), np.zeros((nh, words), np.uint64)
    for k, s in enumerate(sm):
        c, v, inl = hypothesis(job, [int(i) for i in s])
        ni[k], rt[k], bits[k] = c, v, pack_bits(inl)
        if c >= job["min_inliers"]:
            c2, v2, inl2 = refine(job, inl)
            nr[k], rtr[k], rbits[k] = c2, v2, pack_bits(inl2)
    return ni, rt, bits, nr, rtr, rbits


def Tcw_of(rt):
    """mBestTcw / mRefinedTcw: the CV_64F -> CV_32F conversion of :228-234"""
    T = np.eye(4, dtype=f)
    with np.errstate(all="ignore"):
        T[:3, :3] = rt[:9].astype(f).reshape(3, 3)
        T[:3, 3] = rt[9:12].astype(f)
    return T


# ---- SetRansacParameters and iterate

def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """:128-160 -> (mRansacMinInliers, mRansacEpsilon as float32, mRansacMaxIts)"""
    eps = f(epsilon)
    n_min = int(f(N) * eps)                                # int nMinInliers = N*mRansacEpsilon: a float product, truncated
    n_min = max(n_min, min_inliers, min_set)
    with np.errstate(all="ignore"):
        if eps < f(n_min) / f(N):
            eps = f(n_min) / f(N)
        if n_min == N:
            n_it = 1
        else:
            x = np.log(d(1.0) - d(probability)) / np.log(d(1.0) - d(math.pow(float(eps), 3.0)))   # pow(.., 3) although the set has four
            n_it = int(math.ceil(float(x))) if np.isfinite(x) else -2 ** 31
    return n_min, eps, max(1, min(n_it, max_iterations))


def max_error(sigma2, th2=5.991):
    """mvMaxError[i] = mvSigma2[i] * th2, the float product"""
    return (np.asarray(sigma2, f) * f(th2)).astype(f)


class _Ransac:
    """the state PnPsolver keeps between calls.  job: dict(P3Dw, P2D, sigma2, K, samples); the parameters as SetRansacParameters takes them"""

    def __init__(self, job, indices=None, n_matches=None, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4,
                 th2=5.991):
        self.N = len(job["P3Dw"])
        self.indices = np.arange(self.N) if indices is None else np.asarray(indices, np.int64)
        self.n_matches = self.N if n_matches is None else n_matches
        self.min_inliers, self.eps, self.max_its = ransac_parameters(self.N, probability, min_inliers, max_iterations, min_set, epsilon)
        self.job = dict(job, max_err=max_error(job["sigma2"], th2), min_inliers=self.min_inliers)
        self.iterations = 0
        self.best_inliers = 0
        self.best = None          # (Rt, inliers) of the best row
        self.evaluated = 0

    def _scatter(self, inl):
        vb = np.zeros(self.n_matches, bool)
        vb[self.indices[inl]] = True
        return vb

    def iterate(self, n_iterations):
        """-> (Rt[12] or None, bNoMore, vbInliers[n_matches], nInliers)"""
        vb = np.zeros(self.n_matches, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:      # an OR in the reference
            cur += 1
            self.iterations += 1
            k = self.iterations - 1
            ni, rt, inl = self.row(k)
            if ni >= self.min_inliers:
                if ni > self.best_inliers:
                    self.best_inliers, self.best = ni, (rt.copy(), inl.copy())
                    self.new_best(k)
                nr, rtr, inlr = self.refined()
                if nr > self.min_inliers:
                    return rtr, False, self._scatter(inlr), nr
        if self.iterations >= self.max_its:
            if self.best_inliers >= self.min_inliers:
                return self.best[0], True, self._scatter(self.best[1]), self.best_inliers
            return None, True, vb, 0
        return None, False, vb, 0

    def find(self):
        rt, _, vb, ni = self.iterate(self.max_its)
        return rt, vb, ni


class Sequential(_Ransac):
    """the literal loop: hypothesis k is computed when the loop reaches it, and Refine runs on mvbBestInliers every time it is called"""

    def row(self, k):
        self.evaluated += 1
        return hypothesis(self.job, [int(i) for i in np.asarray(self.job["samples"]).reshape(-1, 4)[k]])

    def new_best(self, k):
        pass

    def refined(self):
        return refine(self.job, self.best[1])


class Replay(_Ransac):
    """the mirror's form: a finished table, every qualifying row refined from its own mask; Refine reads the best row's entry"""

    def __init__(self, job, tab, **kw):
        super().__init__(job, **kw)
        self.tab = tab
        self.best_row = -1

    def row(self, k):
        return int(self.tab[0][k]), self.tab[1][k], unpack_bits(self.tab[2][k], self.N)

    def new_best(self, k):
        self.best_row = k

    def refined(self):
        k = self.best_row
        return int(self.tab[3][k]), self.tab[4][k], unpack_bits(self.tab[5][k], self.N)


# ---- the independent evaluation: the same EPnP with numpy.linalg in place of the Jacobi restatements

class Linalg:
    @staticmethod
    def eig(S):
        U, w, _ = np.linalg.svd(S)
        return list(w), [U[:, k] for k in range(len(w))]

    @staticmethod
    def inv(A):
        return np.linalg.inv(A)

    @staticmethod
    def lstsq(A, b):
        return np.linalg.lstsq(A, b, rcond=None)[0]

    @staticmethod
    def uv(A):
        U, _, Vt = np.linalg.svd(A)
        return U, Vt.T


def pose_linalg(job, sample):
    return compute_pose(job, Members(job, sample, True), linalg=Linalg)


def general_position(P):
    """the smallest singular value of the centred sample points (0: coplanar)"""
    P = np.asarray(P, d)
    return float(np.linalg.svd(P - P.mean(0), compute_uv=False)[2])
