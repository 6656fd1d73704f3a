"""numpy float64 restatement of the contract of orbx_local_bundle_adjustment (include/orbx.h): Optimizer::LocalBundleAdjustment (reference
src/Optimizer.cc:528-862) between the optimizer's set-up and vToErase, with the pieces of g2o it runs: EdgeSE3ProjectXYZ /
EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.cpp:103-234), RobustKernelHuber, BaseBinaryEdge::constructQuadraticForm
(base_binary_edge.hpp), BlockSolver_6_3's Schur complement (block_solver.hpp:372-486), OptimizationAlgorithmLevenberg::solve
(optimization_algorithm_levenberg.cpp:61-189), SparseOptimizer::initializeOptimization / optimize (sparse_optimizer.cpp:206-419) and
SE3Quat.  The reduced system is solved by the contract's dense LDL^T (the stated deviation from g2o's SimplicialLDLT).  Every operation
is one numpy operation on float64, rounded on its own.  Written from the reference text; it does not import the library.  The
quaternion, se3_exp, huber and ordered_sum helpers are tests/pose_model.py's.

The sums whose order the contract leaves to the implementation -- Hpp / bp per keyframe, the S and b_S sums, the scale sum, the chi2 sum
over the points -- are taken in one of three orders, "asc", "desc", "pair" (pairwise tree), so that a test can measure how much of a
result is summation noise.  The per-point sums (Hll, bl, a point's chi2, W^T x_p) are in edge order in every variant: the contract fixes them.

optimize(problem, order="asc", stop_at_trial=-1, stop_on_entry=False, mutation=None) -> dict:
  stopped, iterations[2], trials[2], n_level1, n_erase, n_active_kf[2], n_active_points[2], chi2[2], lambda[2], edge_flags[E] (uint8),
  pose [K][3][4] double, point [P][3] double, Tcw [K][4][4] float32, Xw [P][3] float32,
  decisions: one (round, iteration, trial, accepted) per damping trial, lambda_init[2] (computeLambdaInit of each round),
  margin_chi2 / margin_depth: the smallest |chi2 - threshold| and |Pc.z| over the edges at either classification,
  quat_flips: how often SE3Quat::normalizeRotation met w < 0, by call site (pose_model.count_flips).
problem = dict(Tcw [K][4][4], cam [K][5], fixed [K], Xw [P][3], edge_kf, edge_point, x, y, u_right, inv_sigma2)

mutation names one deliberate error (tools/lba_spread.py --mutations measures what each changes):
  "invz_double"      the stereo projection keeps 1 / z in double
  "float_rotation"   a keyframe that has not moved yet maps points with its float rotation block used as a matrix
  "no_lambda_hll"    setLambda skips the Hll blocks
  "reeval_level1"    the final check re-evaluates the level-1 edges at the final estimates
  "lambda_poses"     computeLambdaInit runs over the poses only
"""
import math

import numpy as np

import pose_model as pm
from pose_model import DBL_MAX, DELTA_MONO, DELTA_STEREO, f32, huber, ordered_sum, oplus, pose_from_Tcw, quat_rotate, quat_to_matrix

THR_MONO, THR_STEREO = 5.991, 7.815      # src/Optimizer.cc:761, :777, :805, :820: double comparisons
ORDERS = ("asc", "desc", "pair")
MUTATIONS = ("invz_double", "float_rotation", "no_lambda_hll", "reeval_level1", "lambda_poses")


def seq_sum(v, order):
    """sum of a vector in the named order, every addition rounded (np.cumsum adds one element after the other)"""
    v = np.asarray(v, np.float64)
    if len(v) == 0:
        return 0.0
    if order == "asc":
        return float(np.cumsum(v)[-1])
    if order == "desc":
        return float(np.cumsum(v[::-1])[-1])
    return float(ordered_sum(v, "pair"))


class Groups:
    """terms [T][D] that belong to groups (group[t], kept in the order given) -> the padded index table of group_sum"""

    def __init__(self, group, ngroups):
        group = np.asarray(group, np.int64)
        self.ngroups = ngroups
        cnt = np.bincount(group, minlength=ngroups) if len(group) else np.zeros(ngroups, np.int64)
        self.m = int(cnt.max()) if ngroups and len(group) else 0
        self.idx = np.full((ngroups, max(self.m, 1)), -1, np.int64)
        order = np.argsort(group, kind="stable")
        start = np.concatenate([[0], np.cumsum(cnt)])[:-1] if ngroups else np.zeros(0, np.int64)
        pos = np.arange(len(group)) - np.repeat(start, cnt)
        self.idx[group[order], pos] = order
        self.cnt = cnt

    def sum(self, terms, order):
        """-> [ngroups][D]: every group's terms summed in the named order"""
        D = terms.shape[1:]
        if self.ngroups == 0:
            return np.zeros((0,) + D)
        idx = self.idx
        if order == "desc":                                   # each group's list reversed, still left-aligned
            idx = np.full_like(self.idx, -1)
            for g in range(self.ngroups):
                idx[g, :self.cnt[g]] = self.idx[g, :self.cnt[g]][::-1]
        pad = np.concatenate([terms, np.zeros((1,) + D)])     # index -1: a zero term (adding +0.0 changes nothing)
        cur = pad[idx]                                        # [G][M][D]
        if order in ("asc", "desc"):
            acc = np.zeros((self.ngroups,) + D)
            for k in range(cur.shape[1]):
                acc = acc + cur[:, k]
            return acc
        while cur.shape[1] > 1:
            if cur.shape[1] % 2:
                cur = np.concatenate([cur, np.zeros((self.ngroups, 1) + D)], axis=1)
            cur = cur[:, 0::2] + cur[:, 1::2]
        return cur[:, 0]


def ldlt_solve(S, b):
    """the contract's dense LDL^T on the lower triangle, column by column -> x, or None at a pivot <= 0"""
    n = len(b)
    A = S.copy()
    y = b.copy()
    for j in range(n):
        d = A[j, j]
        if not d > 0.0:
            return None
        l = A[j + 1:, j] / d
        A[j + 1:, j] = l
        y[j + 1:] = y[j + 1:] - l * y[j]
        A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - (l[:, None] * l[None, :]) * d
    y = y / np.diag(A)
    for j in range(n - 1, -1, -1):
        y[:j] = y[:j] - A[j, :j] * y[j]
    return y


class Problem:
    def __init__(self, pr, mutation):
        self.mut = mutation
        self.Tin = np.asarray(pr["Tcw"], f32).reshape(-1, 4, 4)
        self.K = len(self.Tin)
        self.cam = np.asarray(pr["cam"], f32).reshape(-1, 5).astype(np.float64)
        self.fixed = np.asarray(pr["fixed"]).astype(bool)
        self.Xin = np.asarray(pr["Xw"], f32).reshape(-1, 3)
        self.P = len(self.Xin)
        self.ek = np.asarray(pr["edge_kf"], np.int64)
        self.ep = np.asarray(pr["edge_point"], np.int64)
        self.E = len(self.ek)
        g = lambda k: np.asarray(pr[k], f32).astype(np.float64)
        self.mx, self.my, self.mr, self.w = g("x"), g("y"), g("u_right"), g("inv_sigma2")
        self.stereo = ~(np.asarray(pr["u_right"], f32) < f32(0))
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.thr = np.where(self.stereo, THR_STEREO, THR_MONO)
        c = self.cam[self.ek] if self.E else np.zeros((0, 5))
        self.fx, self.fy, self.cx, self.cy, self.bf = [c[:, k] for k in range(5)]
        # rank of an edge among its point's edges (the edges of a point are contiguous)
        self.rank = np.zeros(self.E, np.int64)
        for e in range(1, self.E):
            self.rank[e] = self.rank[e - 1] + 1 if self.ep[e] == self.ep[e - 1] else 0
        self.Rfloat = self.Tin[:, :3, :3].astype(np.float64)

    # ---- estimates: q [K][4], t [K][3], X [P][3], moved [K]
    def start(self):
        q = np.zeros((self.K, 4)); t = np.zeros((self.K, 3))
        for k in range(self.K):
            q[k], t[k] = pose_from_Tcw(self.Tin[k])
        return dict(q=q, t=t, X=self.Xin.astype(np.float64), moved=np.zeros(self.K, bool))

    def camera_points(self, st):
        Pc = quat_rotate(st["q"][self.ek].T, st["X"][self.ep]) + st["t"][self.ek]
        if self.mut == "float_rotation":
            still = ~st["moved"][self.ek]
            dR = self.Rfloat - np.stack([quat_to_matrix(q) for q in st["q"]])
            Pc = Pc + np.where(still[:, None], np.einsum("eij,ej->ei", dR[self.ek], st["X"][self.ep]), 0.0)
        return Pc

    def errors(self, Pc):
        x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
        with np.errstate(all="ignore"):
            invz = 1.0 / z if self.mut == "invz_double" else (1.0 / z).astype(f32).astype(np.float64)
            us = (x * invz) * self.fx + self.cx
            vs = (y * invz) * self.fy + self.cy
            rs = us - self.bf * invz
            um = (x / z) * self.fx + self.cx
            vm = (y / z) * self.fy + self.cy
        e0 = self.mx - np.where(self.stereo, us, um)
        e1 = self.my - np.where(self.stereo, vs, vm)
        e2 = np.where(self.stereo, self.mr - rs, 0.0)
        chi_m = e0 * (self.w * e0) + e1 * (self.w * e1)
        chi_s = chi_m + e2 * (self.w * e2)
        return np.stack([e0, e1, e2], axis=1), np.where(self.stereo, chi_s, chi_m)

    def jac_pose(self, Pc):
        x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
        fx, fy, bf = self.fx, self.fy, self.bf
        z_2 = z * z
        B = np.zeros((self.E, 3, 6))
        B[:, 0, 0] = x * y / z_2 * fx
        B[:, 0, 1] = -(1.0 + (x * x / z_2)) * fx
        B[:, 0, 2] = y / z * fx
        B[:, 0, 3] = -1.0 / z * fx
        B[:, 0, 5] = x / z_2 * fx
        B[:, 1, 0] = (1.0 + y * y / z_2) * fy
        B[:, 1, 1] = -x * y / z_2 * fy
        B[:, 1, 2] = -x / z * fy
        B[:, 1, 4] = -1.0 / z * fy
        B[:, 1, 5] = y / z_2 * fy
        B[:, 2, 0] = B[:, 0, 0] - bf * y / z_2
        B[:, 2, 1] = B[:, 0, 1] + bf * x / z_2
        B[:, 2, 2] = B[:, 0, 2]
        B[:, 2, 3] = B[:, 0, 3]
        B[:, 2, 5] = B[:, 0, 5] - bf / z_2
        B[~self.stereo, 2, :] = 0.0
        return B

    def jac_point(self, st, Pc):
        x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
        fx, fy, bf = self.fx, self.fy, self.bf
        R = np.stack([quat_to_matrix(q) for q in st["q"]])[self.ek]      # [E][3][3]
        z_2 = z * z
        A = np.zeros((self.E, 3, 3))
        s = -1.0 / z
        t00, t01, t02 = s * fx, s * 0.0, s * (-x / z * fx)
        t10, t11, t12 = s * 0.0, s * fy, s * (-y / z * fy)
        for c in range(3):
            a0 = -fx * R[:, 0, c] / z + fx * x * R[:, 2, c] / z_2
            a1 = -fy * R[:, 1, c] / z + fy * y * R[:, 2, c] / z_2
            a2 = a0 - bf * R[:, 2, c] / z_2
            m0 = (t00 * R[:, 0, c] + t01 * R[:, 1, c]) + t02 * R[:, 2, c]
            m1 = (t10 * R[:, 0, c] + t11 * R[:, 1, c]) + t12 * R[:, 2, c]
            A[:, 0, c] = np.where(self.stereo, a0, m0)
            A[:, 1, c] = np.where(self.stereo, a1, m1)
            A[:, 2, c] = np.where(self.stereo, a2, 0.0)
        return A


def three(a0, b0, a1, b1, a2, b2, rw):
    return ((a0 * rw) * b0 + (a1 * rw) * b1) + (a2 * rw) * b2


def optimize(problem, order="asc", stop_at_trial=-1, stop_on_entry=False, mutation=None):
    M = Problem(problem, mutation)
    K, P, E = M.K, M.P, M.E
    res = dict(stopped=0, iterations=[0, 0], trials=[0, 0], n_level1=0, n_erase=0, n_active_kf=[0, 0], n_active_points=[0, 0],
               chi2=[0.0, 0.0], edge_flags=np.zeros(E, np.uint8), decisions=[], margin_chi2=math.inf, margin_depth=math.inf,
               quat_flips={})
    res["lambda"] = [0.0, 0.0]
    res["lambda_init"] = [0.0, 0.0]
    if stop_on_entry:
        res["stopped"] = 1
        return res
    flips = pm.count_flips()
    st = M.start()
    level1 = np.zeros(E, bool)
    echi = np.zeros(E)
    xp_all = np.zeros(6 * 256)                       # the solver's x: a failed solve leaves the previous solution in it
    xl = np.zeros((P, 3))
    trials_total = 0
    evaluated = False
    stop_up = lambda: stop_at_trial >= 0 and trials_total >= stop_at_trial

    def evaluate(state, act, robust):
        """computeActiveErrors -> Pc, err, rho0, rho1 of every edge (only the active ones are used); echi is updated"""
        Pc = M.camera_points(state)
        err, chi = M.errors(Pc)
        echi[act] = chi[act]
        rho0, rho1 = huber(chi, M.delta) if robust else (chi, np.ones(E))
        return Pc, err, rho0, rho1

    def point_chi2(rho0, act, pact):
        c = np.zeros(P)
        for r in range(int(M.rank.max()) + 1 if E else 0):
            idx = np.nonzero(act & (M.rank == r))[0]
            c[M.ep[idx]] = c[M.ep[idx]] + rho0[idx]
        return seq_sum(c[pact], order)

    def classify(state, bit):
        Pc = M.camera_points(state)
        chi = echi
        if mutation == "reeval_level1" and bit == 2:
            chi = np.where(level1, M.errors(Pc)[1], echi)
        bad = (chi > M.thr) | ~(Pc[:, 2] > 0.0)
        if E:
            res["margin_chi2"] = min(res["margin_chi2"], float(np.abs(chi - M.thr).min()))
            res["margin_depth"] = min(res["margin_depth"], float(np.abs(Pc[:, 2]).min()))
        res["edge_flags"][bad] |= bit
        return bad

    for rnd in range(2):
        robust = rnd == 0
        act = ~level1                                                     # the level-0 edges
        kf_act = np.zeros(K, bool)
        kf_act[M.ek[act]] = True
        kf_act &= ~M.fixed
        rowkf = np.nonzero(kf_act)[0]
        row = np.full(K, -1, np.int64)
        row[rowkf] = np.arange(len(rowkf))
        rows, n = len(rowkf), 6 * len(rowkf)
        pact = np.zeros(P, bool)
        pact[M.ep[act]] = True
        res["n_active_kf"][rnd], res["n_active_points"][rnd] = rows, int(pact.sum())
        erow = np.where(act, row[M.ek] if E else 0, -1)                   # the row of an active edge's keyframe, -1: fixed or inactive
        free_e = np.nonzero(erow >= 0)[0]                                 # ascending edges: every keyframe's list in point order
        g_kf = Groups(erow[free_e], rows)
        # the pairs (left edge, right edge) of every block (i, j >= i), in point order
        pl, prr, pb = [], [], []
        blk = lambda i, j: i * rows - i * (i - 1) // 2 + (j - i)
        by_point = {}
        for e in free_e:
            by_point.setdefault(int(M.ep[e]), []).append(int(e))
        for p_ in sorted(by_point):
            es = by_point[p_]
            for a in es:
                for b_ in es:
                    if erow[a] <= erow[b_]:
                        pl.append(a); prr.append(b_); pb.append(blk(int(erow[a]), int(erow[b_])))
        pl, prr = np.array(pl, np.int64), np.array(prr, np.int64)
        nblk = rows * (rows + 1) // 2
        g_blk = Groups(np.array(pb, np.int64), nblk)
        max_rank = int(M.rank.max()) + 1 if E else 0

        lam, ni, n_bad, cur_chi = 0.0, 2.0, 0, 0.0
        for it in range(5 if rnd == 0 else 10):
            if not pact.any() or stop_up():
                break
            # ---- computeActiveErrors + buildSystem at st
            Pc, err, rho0, rho1 = evaluate(st, act, robust)
            evaluated = True
            cur_chi = point_chi2(rho0, act, pact)
            ini_chi = cur_chi
            A = M.jac_point(st, Pc)
            B = M.jac_pose(Pc)
            rw = rho1 * M.w
            omr = -(M.w[:, None] * err) * rho1[:, None]
            Hll = np.zeros((P, 6)); bl = np.zeros((P, 3))
            hl = np.zeros((E, 6)); bt = np.zeros((E, 3))
            q_ = 0
            for r in range(3):
                for c in range(r, 3):
                    hl[:, q_] = three(A[:, 0, r], A[:, 0, c], A[:, 1, r], A[:, 1, c], A[:, 2, r], A[:, 2, c], rw)
                    q_ += 1
                bt[:, r] = (A[:, 0, r] * omr[:, 0] + A[:, 1, r] * omr[:, 1]) + A[:, 2, r] * omr[:, 2]
            for r in range(max_rank):
                idx = np.nonzero(act & (M.rank == r))[0]
                Hll[M.ep[idx]] = Hll[M.ep[idx]] + hl[idx]
                bl[M.ep[idx]] = bl[M.ep[idx]] + bt[idx]
            W = np.zeros((E, 6, 3))
            for r in range(6):
                for c in range(3):
                    W[:, r, c] = three(B[:, 0, r], A[:, 0, c], B[:, 1, r], A[:, 1, c], B[:, 2, r], A[:, 2, c], rw)
            kt = np.zeros((len(free_e), 27))
            q_ = 0
            Bf, rwf, omf = B[free_e], rw[free_e], omr[free_e]
            for r in range(6):
                for c in range(r, 6):
                    kt[:, q_] = three(Bf[:, 0, r], Bf[:, 0, c], Bf[:, 1, r], Bf[:, 1, c], Bf[:, 2, r], Bf[:, 2, c], rwf)
                    q_ += 1
                kt[:, 21 + r] = (Bf[:, 0, r] * omf[:, 0] + Bf[:, 1, r] * omf[:, 1]) + Bf[:, 2, r] * omf[:, 2]
            ks = g_kf.sum(kt, order)
            Hpp, bp = ks[:, :21], ks[:, 21:]
            if it == 0:
                md = 0.0
                if rows:
                    md = max(md, float(np.abs(Hpp[:, [0, 6, 11, 15, 18, 20]]).max()))
                if mutation != "lambda_poses":
                    md = max(md, float(np.abs(Hll[pact][:, [0, 3, 5]]).max()))
                lam, ni, n_bad = 1e-5 * md, 2.0, 0
                res["lambda_init"][rnd] = lam
            rho, qmax = 0.0, 0
            while True:
                # ---- setLambda, the Schur complement, the solve
                lh = 0.0 if mutation == "no_lambda_hll" else lam
                m00, m01, m02, m11, m12, m22 = Hll[:, 0] + lh, Hll[:, 1], Hll[:, 2], Hll[:, 3] + lh, Hll[:, 4], Hll[:, 5] + lh
                with np.errstate(all="ignore"):
                    c00, c01, c02 = m11 * m22 - m12 * m12, m12 * m02 - m01 * m22, m01 * m12 - m11 * m02
                    c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
                    det = (c00 * m00 + c01 * m01) + c02 * m02
                    inv = 1.0 / det
                    D = np.zeros((P, 3, 3))
                    D[:, 0, 0], D[:, 0, 1], D[:, 0, 2] = c00 * inv, c01 * inv, c02 * inv
                    D[:, 1, 0], D[:, 1, 1], D[:, 1, 2] = D[:, 0, 1], c11 * inv, c12 * inv
                    D[:, 2, 0], D[:, 2, 1], D[:, 2, 2] = D[:, 0, 2], D[:, 1, 2], c22 * inv
                D[~pact] = 0.0
                db = np.stack([(D[:, r, 0] * bl[:, 0] + D[:, r, 1] * bl[:, 1]) + D[:, r, 2] * bl[:, 2] for r in range(3)], axis=1)
                ok = True
                if rows:
                    Wi, Wj, Dp = W[pl], W[prr], D[M.ep[pl]]
                    BD = np.zeros((len(pl), 6, 3))
                    for c in range(3):
                        BD[:, :, c] = (Wi[:, :, 0] * Dp[:, None, 0, c] + Wi[:, :, 1] * Dp[:, None, 1, c]) + Wi[:, :, 2] * Dp[:, None, 2, c]
                    T = np.zeros((len(pl), 6, 6))
                    for c in range(6):
                        T[:, :, c] = (BD[:, :, 0] * Wj[:, None, c, 0] + BD[:, :, 1] * Wj[:, None, c, 1]) + BD[:, :, 2] * Wj[:, None, c, 2]
                    bs = g_blk.sum(T, order)
                    Wf, dbf = W[free_e], db[M.ep[free_e]]
                    bterm = (Wf[:, :, 0] * dbf[:, None, 0] + Wf[:, :, 1] * dbf[:, None, 1]) + Wf[:, :, 2] * dbf[:, None, 2]
                    bsum = g_kf.sum(bterm, order)
                    S = np.zeros((n, n)); bS = np.zeros(n)
                    for i in range(rows):
                        Hu = np.zeros((6, 6))
                        Hu[np.triu_indices(6)] = Hpp[i]
                        Hu = Hu + lam * np.eye(6)
                        blk_ii = Hu - bs[blk(i, i)]
                        up = np.triu(blk_ii)
                        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = up + np.triu(blk_ii, 1).T
                        bS[6 * i:6 * i + 6] = bp[i] - bsum[i]
                        for j in range(i + 1, rows):
                            v = 0.0 - bs[blk(i, j)]
                            S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = v
                            S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = v.T
                    sol = ldlt_solve(S, bS)
                    ok = sol is not None
                    if ok:
                        xp_all[:n] = sol
                xp = xp_all[:n].reshape(rows, 6) if rows else np.zeros((0, 6))
                if ok:
                    cvec = bl.copy()
                    for r in range(max_rank):
                        idx = np.nonzero((erow >= 0) & (M.rank == r))[0]
                        xe = xp[erow[idx]]
                        Wt = W[idx]
                        s_ = Wt[:, 0, :] * xe[:, None, 0]
                        for k_ in range(1, 6):
                            s_ = s_ + Wt[:, k_, :] * xe[:, None, k_]
                        cvec[M.ep[idx]] = cvec[M.ep[idx]] - s_
                    new_xl = np.stack([(D[:, r, 0] * cvec[:, 0] + D[:, r, 1] * cvec[:, 1]) + D[:, r, 2] * cvec[:, 2] for r in range(3)], axis=1)
                    xl[pact] = new_xl[pact]
                # ---- update into the trial copy (push)
                trial = dict(q=st["q"].copy(), t=st["t"].copy(), X=st["X"].copy(), moved=st["moved"].copy())
                for r_, k_ in enumerate(rowkf):
                    trial["q"][k_], trial["t"][k_] = oplus((st["q"][k_], st["t"][k_]), xp[r_])
                    trial["moved"][k_] = True
                trial["X"][pact] = st["X"][pact] + xl[pact]
                _, _, trho0, _ = evaluate(trial, act, robust)
                temp = point_chi2(trho0, act, pact) if ok else DBL_MAX
                sterms = np.concatenate([(xp * (lam * xp + bp)).reshape(-1), (xl[pact] * (lam * xl[pact] + bl[pact])).reshape(-1)])
                scale = seq_sum(sterms, order) + 1e-3
                trials_total += 1
                res["trials"][rnd] += 1
                with np.errstate(all="ignore"):
                    rho = float((np.float64(cur_chi) - np.float64(temp)) / np.float64(scale))
                accepted = rho > 0.0 and math.isfinite(temp)
                res["decisions"].append((rnd, it, qmax, accepted))
                if accepted:
                    t_ = 2.0 * rho - 1.0
                    alpha = min(1.0 - (t_ * t_) * t_, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur_chi = temp
                    st = trial
                else:
                    lam *= ni
                    ni *= 2.0
                qmax += 1
                if not (rho < 0.0 and qmax < 10 and not stop_up()):
                    break
            res["iterations"][rnd] += 1
            if qmax == 10 or rho == 0.0:
                break
            n_bad = n_bad + 1 if (ini_chi - cur_chi) * 1e3 < ini_chi else 0
            if n_bad >= 3:
                break
        res["chi2"][rnd], res["lambda"][rnd] = cur_chi, lam
        if rnd == 0:
            if stop_up():
                res["stopped"] = 2
            if not evaluated and E:
                evaluate(st, act, True)
                evaluated = True
            level1 = classify(st, 1)
            if res["stopped"]:
                break
        elif stop_up():
            res["stopped"] = 3
    classify(st, 2)
    res["n_level1"] = int((res["edge_flags"] & 1).sum())
    res["n_erase"] = int(((res["edge_flags"] >> 1) & 1).sum())
    pose = np.zeros((K, 3, 4))
    for k in range(K):
        pose[k, :, :3] = quat_to_matrix(st["q"][k])
        pose[k, :, 3] = st["t"][k]
    T = np.zeros((K, 4, 4), f32)
    T[:, :3, :] = pose.astype(f32)
    T[:, 3, 3] = 1
    res["pose"], res["point"], res["Tcw"], res["Xw"] = pose, st["X"].copy(), T, st["X"].astype(f32)
    res["quat_flips"] = dict(flips)
    return res
