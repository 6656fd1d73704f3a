"""numpy float64 restatement of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1164-1365) with the pieces of g2o it runs: g2o::Sim3
(Thirdparty/g2o/g2o/types/sim3.h), VertexSim3Expmap / EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (types_seven_dof_expmap.h:60-171), the
numeric BaseBinaryEdge::linearizeOplus and constructQuadraticForm (base_binary_edge.hpp:55-205), RobustKernelHuber, LinearSolverDense,
OptimizationAlgorithmLevenberg::solve and SparseOptimizer::optimize.  Written from the reference text, independently of the kernel; Huber,
Eigen's quaternion pieces and the ordered sums are tests/pose_model.py's.  It does not import the library.

optimize(obs, cam1, cam2, S12, th2, fix_scale, order, nudge, jacobian, mutant) -> dict.  The switches:

  variants (none of them an error; the spread between them is what a faithful implementation may differ by)
    order     "asc" | "desc" | "pair": the summation order of the 28 + 7 + 1 sums over the edges (pose_model.ordered_sum)
    nudge     None, or a seed: every sin, cos and exp result inside the Sim3 exponential is moved one ulp up or down by a seeded pattern
              (a C library and a device library differ like that).  Results that every library gives exactly -- sin(0), cos(0), exp(0) --
              are left alone: with fix_scale the whole of column 6 rests on exp(0) == 1.
    jacobian  "numeric": the reference's central difference; "closed": the derivative it approximates, in closed form

  mutants (each one a real error; tests/test_sim3opt_model.py shows that the test bound tells them from the truth)
    "edge21_forward"   edge 21 mapped with S12 instead of its inverse
    "cams_swapped"     cam1 and cam2 exchanged
    "fix_scale_off"    fix_scale ignored
    "round2_restart"   round 2 restarted from the input estimate
    "huber_th2"        Huber delta = th2 instead of its square root
    "normalise"        the quaternion normalised to unit length after operator*

Result: n_corr, rounds, n_bad, more_iterations, iterations[2], chi2[2] (the active robust chi2 each round ended with), ret, S12[8] (the
function's g2oS12 on return: the input on a return of 0), estimate[8] (where the optimiser stood), inlier[n] (uint8: vpMatches1[i] still
non-NULL; 0 where no pair), idx[n_corr], class_chi2[rounds] ([k][2]: chi2_12, chi2_21 of every pair each classification looked at) with
class_idx[rounds] (their feature indices), decisions (round, iteration, trial, accepted, currentChi, tempChi, max |x_j|) and stale_used."""
import math

import numpy as np

import pose_model as pm

f32 = np.float32
DBL_MAX = pm.DBL_MAX
MUTANTS = ("edge21_forward", "cams_swapped", "fix_scale_off", "round2_restart", "huber_th2", "normalise")
DELTA = 1e-9                                   # base_binary_edge.hpp:147
SCALAR = 1.0 / (2 * DELTA)


class Libm:
    """sin, cos, exp; with a seed, each result one ulp up or down by a seeded pattern (exact results stay)"""

    def __init__(self, seed=None):
        self.rng = None if seed is None else np.random.Generator(np.random.PCG64(seed))

    def _n(self, v, exact):
        if self.rng is None:
            return v
        up = self.rng.integers(0, 2) == 1       # drawn on every call, so the pattern does not depend on the arguments
        return v if exact else float(np.nextafter(v, math.inf if up else -math.inf))

    def sin(self, x):
        return self._n(math.sin(x), x == 0.0)

    def cos(self, x):
        return self._n(math.cos(x), x == 0.0)

    def exp(self, x):
        return self._n(math.exp(x), x == 0.0)


# ---------------------------------------------------------------- g2o::Sim3 as (q = (x, y, z, w), t, s); q is never normalised

def sim3_from8(v):
    v = np.asarray(v, np.float64).reshape(8)
    return v[:4].copy(), v[4:7].copy(), float(v[7])


def sim3_to8(S):
    return np.concatenate([S[0], S[1], [S[2]]])


def sim3_exp(u, lm):
    """sim3.h:70-142"""
    o, ups, sigma = u[:3], u[3:6], float(u[6])
    theta = math.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    O = np.array([[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]])
    O2 = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            O2[r, c] = (O[r, 0] * O[0, c] + O[r, 1] * O[1, c]) + O[r, 2] * O[2, c]
    s = lm.exp(sigma)
    I = np.eye(3)
    eps = 0.00001
    if theta < eps:
        R = (I + O) + O2
    else:
        sn, cs = lm.sin(theta), lm.cos(theta)
        R = (I + sn / theta * O) + (1.0 - cs) / (theta * theta) * O2
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            theta2 = theta * theta
            A = (1.0 - lm.cos(theta)) / theta2
            B = (theta - lm.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
        else:
            a, b = s * lm.sin(theta), s * lm.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2
    W = (A * O + B * O2) + C * I
    t = np.array([(W[r, 0] * ups[0] + W[r, 1] * ups[1]) + W[r, 2] * ups[2] for r in range(3)])
    return pm.quat_from_matrix(R), t, s


def sim3_map(S, P):
    """sim3.h:144-146; P is [..., 3]"""
    q, t, s = S
    return s * pm.quat_rotate(q, P) + t


def sim3_inverse(S):
    """sim3.h:233-236"""
    q, t, s = S
    qc = np.array([-q[0], -q[1], -q[2], q[3]])
    return qc, pm.quat_rotate(qc, (-1.0 / s) * t), 1.0 / s


def sim3_mul(a, b, normalise=False):
    """sim3.h:266-272: no normalisation of the product (the mutant adds SE3Quat's)"""
    (aq, at, as_), (bq, bt, bs) = a, b
    ax, ay, az, aw = aq
    bx, by, bz, bw = bq
    q = np.array([((aw * bx + ax * bw) + ay * bz) - az * by,
                  ((aw * by + ay * bw) + az * bx) - ax * bz,
                  ((aw * bz + az * bw) + ax * by) - ay * bx,
                  ((aw * bw - ax * bx) - ay * by) - az * bz])
    if normalise:
        q = pm.quat_normalize(q)
    return q, as_ * pm.quat_rotate(aq, bt) + at, as_ * bs


# ---------------------------------------------------------------- edges

class Pairs:
    """the correspondences in feature order, widened to double; edge 12 and edge 21 of pair k are edges 2k and 2k + 1"""

    def __init__(self, obs, cam1, cam2, mutant):
        has = np.asarray(obs["has_pair"]).astype(bool)
        self.idx = np.nonzero(has)[0]
        self.n = len(self.idx)
        g = lambda k: np.asarray(obs[k], f32)[self.idx].astype(np.float64)
        self.P1 = np.asarray(obs["P1c"], f32).reshape(-1, 3)[self.idx].astype(np.float64)
        self.P2 = np.asarray(obs["P2c"], f32).reshape(-1, 3)[self.idx].astype(np.float64)
        self.m1 = np.stack([g("x1"), g("y1")], axis=1) if self.n else np.zeros((0, 2))
        self.m2 = np.stack([g("x2"), g("y2")], axis=1) if self.n else np.zeros((0, 2))
        self.w1, self.w2 = g("inv_sigma2_1"), g("inv_sigma2_2")
        k1 = [float(v) for v in np.asarray(cam1, f32)[:4]]
        k2 = [float(v) for v in np.asarray(cam2, f32)[:4]]
        self.K1, self.K2 = (k2, k1) if mutant == "cams_swapped" else (k1, k2)
        self.forward21 = mutant == "edge21_forward"

    @staticmethod
    def _err(T, K, P, m, w):
        Pc = sim3_map(T, P)
        with np.errstate(all="ignore"):
            e0 = m[:, 0] - ((Pc[:, 0] / Pc[:, 2]) * K[0] + K[2])
            e1 = m[:, 1] - ((Pc[:, 1] / Pc[:, 2]) * K[1] + K[3])
        return np.stack([e0, e1], axis=1), e0 * (w * e0) + e1 * (w * e1), Pc

    def errors(self, S):
        """-> (e12 [n][2], chi12 [n], Pc12), (e21, chi21, Pc21)"""
        return self._err(S, self.K1, self.P2, self.m1, self.w1), \
            self._err(S if self.forward21 else sim3_inverse(S), self.K2, self.P1, self.m2, self.w2)

    def jacobians_numeric(self, S, fix, lm, normalise):
        """base_binary_edge.hpp:176-198 -> A12 [n][2][7], A21 [n][2][7]"""
        A12, A21 = np.zeros((self.n, 2, 7)), np.zeros((self.n, 2, 7))
        for d in range(7):
            side = []
            for sign in (1.0, -1.0):
                u = np.zeros(7)
                u[d] = sign * DELTA
                if fix:
                    u[6] = 0.0                                            # oplusImpl
                (e12, _, _), (e21, _, _) = self.errors(sim3_mul(sim3_exp(u, lm), S, normalise))
                side.append((e12, e21))
            A12[:, :, d] = SCALAR * (side[0][0] - side[1][0])
            A21[:, :, d] = SCALAR * (side[0][1] - side[1][1])
        return A12, A21

    def jacobians_closed(self, S, fix):
        """what the central difference approximates: d/du of the errors at exp(u) * S, u = 0.  exp(u) maps p to p + omega x p + upsilon +
        sigma p to first order; (exp(u) S)^-1 = S^-1 exp(-u), and S^-1's linear part is (1 / s) M(conj q)"""
        def dproj(Pc, K):
            x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
            D = np.zeros((len(Pc), 2, 3))
            D[:, 0, 0] = K[0] / z; D[:, 0, 2] = -K[0] * x / (z * z)
            D[:, 1, 1] = K[1] / z; D[:, 1, 2] = -K[1] * y / (z * z)
            return D

        def dpoint(p):
            """[n][3][7]: -[p]x | I | p"""
            G = np.zeros((len(p), 3, 7))
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            G[:, 0, 1] = z; G[:, 0, 2] = -y; G[:, 1, 0] = -z; G[:, 1, 2] = x; G[:, 2, 0] = y; G[:, 2, 1] = -x
            G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
            G[:, :, 6] = p
            return G

        (_, _, Pc12), (_, _, Pc21) = self.errors(S)
        A12 = -np.einsum("nij,njk->nik", dproj(Pc12, self.K1), dpoint(Pc12))
        if self.forward21:
            A21 = -np.einsum("nij,njk->nik", dproj(Pc21, self.K2), dpoint(Pc21))
        else:
            q, _, s = S
            qc = np.array([-q[0], -q[1], -q[2], q[3]])
            G = dpoint(self.P1)
            lin = np.stack([pm.quat_rotate(qc, G[:, :, k]) for k in range(7)], axis=2) / s
            A21 = np.einsum("nij,njk->nik", dproj(Pc21, self.K2), lin)
        if fix:
            A12[:, :, 6] = 0.0
            A21[:, :, 6] = 0.0
        return A12, A21


def solve_ldl(H, b, lam):
    """(H + lam I) x = b by LDL^T without pivoting -> x, or None unless every pivot is > 0 (linear_solver_dense.h:104-112)"""
    n = len(b)
    A = H + lam * np.eye(n)
    L = np.zeros((n, n))
    d = np.zeros(n)
    for j in range(n):
        dj = A[j, j]
        for m in range(j):
            dj -= (L[j, m] * L[j, m]) * d[m]
        if not dj > 0.0:
            return None
        d[j] = dj
        for i in range(j + 1, n):
            v = A[i, j]
            for m in range(j):
                v -= (L[i, m] * L[j, m]) * d[m]
            L[i, j] = v / dj
    y = np.zeros(n)
    for i in range(n):
        v = b[i]
        for m in range(i):
            v -= L[i, m] * y[m]
        y[i] = v
    y = y / d
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        v = y[i]
        for m in range(i + 1, n):
            v -= L[m, i] * x[m]
        x[i] = v
    return x


def edge_terms(A, err, chi2, w, delta):
    """one edge type's contribution per pair -> [n][36]: H's upper triangle, b, rho0 (base_binary_edge.hpp:91-113)"""
    rho0, rho1 = pm.huber(chi2, delta)
    rw = rho1 * w
    we = w[:, None] * err
    T = np.zeros((len(chi2), 36))
    k = 0
    for r in range(7):
        for c in range(r, 7):
            T[:, k] = (A[:, 0, r] * rw) * A[:, 0, c] + (A[:, 1, r] * rw) * A[:, 1, c]
            k += 1
        T[:, 28 + r] = -(rho1 * (A[:, 0, r] * we[:, 0] + A[:, 1, r] * we[:, 1]))
    T[:, 35] = rho0
    return T


def optimize(obs, cam1, cam2, S12, th2, fix_scale, order="asc", nudge=None, jacobian="numeric", mutant=None):
    assert mutant is None or mutant in MUTANTS
    E = Pairs(obs, cam1, cam2, mutant)
    lm = Libm(nudge)
    n = len(np.asarray(obs["has_pair"]))
    th2 = f32(th2)
    thr = float(th2)                                                      # :1317: a double against the float, widened
    delta = thr if mutant == "huber_th2" else float(f32(math.sqrt(th2)))  # :1217: const float deltaHuber = sqrt(th2)
    fix = bool(fix_scale) and mutant != "fix_scale_off"
    normalise = mutant == "normalise"
    start = sim3_from8(S12)
    res = dict(n_corr=E.n, rounds=0, n_bad=0, more_iterations=5, iterations=[0, 0], chi2=[0.0, 0.0], ret=0, idx=E.idx,
               S12=sim3_to8(start), estimate=sim3_to8(start), inlier=np.zeros(n, np.uint8), class_chi2=[], class_idx=[], decisions=[],
               stale_used=False)
    if E.n == 0:
        return res
    active = np.ones(E.n, bool)
    S = start
    x = np.zeros(7)

    def system(S):
        (e12, c12, _), (e21, c21, _) = E.errors(S)
        A12, A21 = E.jacobians_numeric(S, fix, lm, normalise) if jacobian == "numeric" else E.jacobians_closed(S, fix)
        T = np.zeros((2 * E.n, 36))
        T[0::2] = edge_terms(A12, e12, c12, E.w1, delta)
        T[1::2] = edge_terms(A21, e21, c21, E.w2, delta)
        s = pm.ordered_sum(T[np.repeat(active, 2)], order)
        H = np.zeros((7, 7))
        k = 0
        for r in range(7):
            for c in range(r, 7):
                H[r, c] = H[c, r] = s[k]
                k += 1
        return H, s[28:35].copy(), float(s[35])

    def robust_chi2(S):
        (_, c12, _), (_, c21, _) = E.errors(S)
        T = np.zeros(2 * E.n)
        T[0::2] = pm.huber(c12, delta)[0]
        T[1::2] = pm.huber(c21, delta)[0]
        return float(pm.ordered_sum(T[np.repeat(active, 2)], order)), np.stack([c12, c21], axis=1)

    for rnd in range(2):
        if rnd == 1 and mutant == "round2_restart":
            S = start
        max_iter = 5 if rnd == 0 else res["more_iterations"]
        lam, ni, stop_bad, iters, cur = 0.0, 2.0, 0, 0, 0.0
        trial_chi2, last_rejected = None, False
        for iteration in range(max_iter):
            H, b, cur = system(S)
            ini = cur
            if iteration == 0:
                lam, ni, stop_bad = 1e-5 * max(0.0, *[abs(H[j, j]) for j in range(7)]), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                backup = S
                sol = solve_ldl(H, b, lam)
                if sol is not None:
                    x = sol
                if fix:
                    x[6] = 0.0                                            # oplusImpl writes into the solver's x
                S = sim3_mul(sim3_exp(x, lm), S, normalise)
                temp, trial_chi2 = robust_chi2(S)
                if sol is None:
                    temp = DBL_MAX
                scale = 0.0
                for j in range(7):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                with np.errstate(all="ignore"):
                    rho = float((np.float64(cur) - np.float64(temp)) / np.float64(scale))
                accepted = rho > 0.0 and math.isfinite(temp)
                res["decisions"].append((rnd, iteration, qmax, accepted, cur, temp, float(np.abs(x).max())))
                if accepted:
                    t = 2.0 * rho - 1.0
                    alpha = min(1.0 - (t * t) * t, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur = temp
                else:
                    lam *= ni
                    ni *= 2.0
                    S = backup                                            # pop(): the vertex only
                last_rejected = not accepted
                qmax += 1
                if not (rho < 0.0 and qmax < 10):
                    break
            iters += 1
            if qmax == 10 or rho == 0.0:
                break
            stop_bad = stop_bad + 1 if (ini - cur) * 1e3 < ini else 0
            if stop_bad >= 3:
                break
        # :1308-1327 / :1343-1358: the pairs still in the graph, at the errors of the last evaluated trial
        res["stale_used"] = res["stale_used"] or last_rejected
        bad = active & ((trial_chi2[:, 0] > thr) | (trial_chi2[:, 1] > thr))
        res["class_chi2"].append(trial_chi2[active].copy())
        res["class_idx"].append(E.idx[active].copy())
        active = active & ~bad
        res["iterations"][rnd] = iters
        res["chi2"][rnd] = cur
        res["rounds"] = rnd + 1
        res["estimate"] = sim3_to8(S)
        if rnd == 0:
            res["n_bad"] = int(bad.sum())
            res["more_iterations"] = 10 if res["n_bad"] > 0 else 5
            if E.n - res["n_bad"] < 10:                                   # :1335-1336
                break
    res["inlier"][E.idx] = active
    if res["rounds"] == 2:
        res["S12"] = sim3_to8(S)
        res["ret"] = int(active.sum())
    return res


def sim3_matrix(S8):
    """[s R | t] of an S12 as 3 x 4, R by Eigen's toRotationMatrix of the quaternion as it stands -- what tools/pose_spread.py's pose_diff
    compares -- and s"""
    q, t, s = sim3_from8(S8)
    return np.concatenate([s * pm.quat_to_matrix(q), t[:, None]], axis=1), s


def same_path(results):
    a = [d[:4] for d in results[0]["decisions"]]
    return all([d[:4] for d in r["decisions"]] == a for r in results[1:])
