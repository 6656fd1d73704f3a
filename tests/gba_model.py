"""numpy float64 restatement of the contract of orbx_bundle_adjustment (include/orbx.h): Optimizer::BundleAdjustment (reference
src/Optimizer.cc:48-281) between the optimizer's set-up (:67) and the recovery loops (:232).  The per-edge and per-point arithmetic is
tests/lba_model.py's (Problem, Groups, seq_sum, three, ldlt_solve are imported from it); what is restated here is the loop: ONE round of
`iterations` Levenberg iterations on every edge, Huber throughout if `robust`, no classification, no levels, no return on entry.

optimize(problem, iterations=10, robust=True, order="asc", stop_at_trial=-1, stop_on_entry=False, mutation=None) -> dict:
  stopped (0, 1 = the flag was up on entry, 2 = it rose during the round), iterations, trials, n_active_kf, n_active_points, chi2, lambda,
  lambda_init, point_included [P] uint8, pose [K][3][4] double, point [P][3] double, Tcw [K][4][4] float32, Xw [P][3] float32,
  decisions: one (iteration, trial, accepted) per damping trial, quat_flips (pose_model.count_flips).
The sums whose order the contract leaves open are taken in `order`, one of lba_model.ORDERS.

mutation names one deliberate error (tools/gba_spread.py --mutations measures what each changes):
  "invz_double", "float_rotation", "no_lambda_hll", "lambda_poses"   as in lba_model
  "no_huber"         the edges carry no robust kernel although robust is set
  "huber_5991"       a monocular edge's Huber delta is LocalBundleAdjustment's (float)sqrt(5.991)

ldlt_blocked(S, b, width): the same LDL^T as lba_model.ldlt_solve, computed panel by panel as orbx_ldlt.hip does (diagonal block, the
panel's rows, the trailing matrix, the backward substitution in blocks).  Every entry sees the same operations in the same order, so the
result is the same bytes."""
import math

import numpy as np

from lba_model import ORDERS, Groups, Problem, ldlt_solve, seq_sum, three  # noqa: F401  (ORDERS, ldlt_solve: for the users of this module)
from pose_model import DBL_MAX, DELTA_MONO, DELTA_STEREO, count_flips, f32, huber, oplus, quat_to_matrix

DELTA_MONO_BA = float(f32(math.sqrt(5.99)))      # src/Optimizer.cc:101 thHuber2D = sqrt(5.99): not LocalBundleAdjustment's 5.991
MUTATIONS = ("invz_double", "float_rotation", "no_lambda_hll", "lambda_poses", "no_huber", "huber_5991")


def ldlt_blocked(S, b, width):
    """-> x, or None at a pivot that is not > 0"""
    n = len(b)
    A = S.copy()
    y = b.copy()
    for j0 in range(0, n, width):
        j1 = min(j0 + width, n)
        for j in range(j0, j1):                                  # the diagonal block, with its part of y
            d = A[j, j]
            if not d > 0.0:
                return None
            l = A[j + 1:j1, j] / d
            A[j + 1:j1, j] = l
            y[j + 1:j1] = y[j + 1:j1] - l * y[j]
            A[j + 1:j1, j + 1:j1] = A[j + 1:j1, j + 1:j1] - (l[:, None] * l[None, :]) * d
        for j in range(j0, j1):                                  # the rows below it: their entries of L, their y
            d = A[j, j]
            l = A[j1:, j] / d
            A[j1:, j] = l
            y[j1:] = y[j1:] - l * y[j]
            A[j1:, j + 1:j1] = A[j1:, j + 1:j1] - (l[:, None] * A[j + 1:j1, j][None, :]) * d
        for j in range(j0, j1):                                  # the trailing matrix, the panel's columns one after the other
            l = A[j1:, j]
            A[j1:, j1:] = A[j1:, j1:] - (l[:, None] * l[None, :]) * A[j, j]
    y = y / np.diag(A)
    for j0 in range((n - 1) // width * width, -1, -width):
        j1 = min(j0 + width, n)
        for j in range(j1 - 1, j0 - 1, -1):                      # the panel's unknowns
            y[j0:j] = y[j0:j] - A[j, j0:j] * y[j]
        for j in range(j1 - 1, j0 - 1, -1):                      # taken out of the rows above
            y[:j0] = y[:j0] - A[j, :j0] * y[j]
    return y


def optimize(problem, iterations=10, robust=True, order="asc", stop_at_trial=-1, stop_on_entry=False, mutation=None):
    M = Problem(problem, mutation)
    M.delta = np.where(M.stereo, DELTA_STEREO, DELTA_MONO if mutation == "huber_5991" else DELTA_MONO_BA)
    K, P, E = M.K, M.P, M.E
    robust = bool(robust) and mutation != "no_huber"
    res = dict(stopped=0, iterations=0, trials=0, chi2=0.0, lambda_init=0.0, decisions=[])
    res["lambda"] = 0.0
    flips = count_flips()
    st = M.start()
    kf_act = np.zeros(K, bool)
    kf_act[M.ek] = True
    kf_act &= ~M.fixed
    rowkf = np.nonzero(kf_act)[0]
    row = np.full(K, -1, np.int64)
    row[rowkf] = np.arange(len(rowkf))
    rows, n = len(rowkf), 6 * len(rowkf)
    pact = np.zeros(P, bool)
    pact[M.ep] = True
    res["n_active_kf"], res["n_active_points"] = rows, int(pact.sum())
    res["point_included"] = pact.astype(np.uint8)
    erow = row[M.ek] if E else np.zeros(0, np.int64)
    free_e = np.nonzero(erow >= 0)[0]
    g_kf = Groups(erow[free_e], rows)
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
    g_blk = Groups(np.array(pb, np.int64), rows * (rows + 1) // 2)
    max_rank = int(M.rank.max()) + 1 if E else 0
    xp_all = np.zeros(n)                                         # a failed solve leaves the previous solution in it
    xl = np.zeros((P, 3))
    trials_total = 0
    stop_up = lambda: stop_at_trial >= 0 and trials_total >= stop_at_trial

    def evaluate(state):
        Pc = M.camera_points(state)
        err, chi = M.errors(Pc)
        rho0, rho1 = huber(chi, M.delta) if robust else (chi, np.ones(E))
        return Pc, err, rho0, rho1

    def point_chi2(rho0):
        c = np.zeros(P)
        for r in range(max_rank):
            idx = np.nonzero(M.rank == r)[0]
            c[M.ep[idx]] = c[M.ep[idx]] + rho0[idx]
        return seq_sum(c[pact], order)

    lam, ni, n_bad, cur_chi = 0.0, 2.0, 0, 0.0
    for it in range(0 if stop_on_entry else iterations):
        if not pact.any() or stop_up():
            break
        Pc, err, rho0, rho1 = evaluate(st)
        cur_chi = point_chi2(rho0)
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
            idx = np.nonzero(M.rank == r)[0]
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
            res["lambda_init"] = lam
        rho, qmax = 0.0, 0
        while True:
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
                S = (0.0 - bs).reshape(-1, 6, 6)                                   # block (i, j >= i) at blk(i, j)
                Sm = np.zeros((n, n)); bS = np.zeros(n)
                iu, ju = np.triu_indices(rows)
                Sv = Sm.reshape(rows, 6, rows, 6)
                Sv[iu, :, ju, :] = S
                Sv[ju, :, iu, :] = S.transpose(0, 2, 1)
                for i in range(rows):
                    Hu = np.zeros((6, 6))
                    Hu[np.triu_indices(6)] = Hpp[i]
                    Hu = Hu + lam * np.eye(6)
                    blk_ii = Hu - bs[blk(i, i)]
                    Sm[6 * i:6 * i + 6, 6 * i:6 * i + 6] = np.triu(blk_ii) + np.triu(blk_ii, 1).T
                    bS[6 * i:6 * i + 6] = bp[i] - bsum[i]
                sol = ldlt_solve(Sm, bS)
                ok = sol is not None
                if ok:
                    xp_all[:] = sol
            xp = xp_all.reshape(rows, 6)
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
            trial = dict(q=st["q"].copy(), t=st["t"].copy(), X=st["X"].copy(), moved=st["moved"].copy())
            for r_, k_ in enumerate(rowkf):
                trial["q"][k_], trial["t"][k_] = oplus((st["q"][k_], st["t"][k_]), xp[r_])
                trial["moved"][k_] = True
            trial["X"][pact] = st["X"][pact] + xl[pact]
            _, _, trho0, _ = evaluate(trial)
            temp = point_chi2(trho0) if ok else DBL_MAX
            sterms = np.concatenate([(xp * (lam * xp + bp)).reshape(-1), (xl[pact] * (lam * xl[pact] + bl[pact])).reshape(-1)])
            scale = seq_sum(sterms, order) + 1e-3
            trials_total += 1
            res["trials"] += 1
            with np.errstate(all="ignore"):
                rho = float((np.float64(cur_chi) - np.float64(temp)) / np.float64(scale))
            accepted = rho > 0.0 and math.isfinite(temp)
            res["decisions"].append((it, qmax, accepted))
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
        res["iterations"] += 1
        if qmax == 10 or rho == 0.0:
            break
        n_bad = n_bad + 1 if (ini_chi - cur_chi) * 1e3 < ini_chi else 0
        if n_bad >= 3:
            break
    res["chi2"], res["lambda"] = cur_chi, lam
    res["stopped"] = 1 if stop_on_entry else (2 if stop_up() else 0)
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
