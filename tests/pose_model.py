"""numpy float64 restatement of Optimizer::PoseOptimization (reference src/Optimizer.cc:286-513) with the pieces of g2o it runs:
EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose (types_six_dof_expmap.cpp:266-364), RobustKernelHuber
(robust_kernel_impl.cpp:78-91), BaseUnaryEdge::constructQuadraticForm (base_unary_edge.hpp:43-72), OptimizationAlgorithmLevenberg::solve
(optimization_algorithm_levenberg.cpp:61-189), LinearSolverDense (linear_solver_dense.h:104-112), SE3Quat (se3quat.h) and
SparseOptimizer::optimize (sparse_optimizer.cpp:354-419).  Written from the reference text; it does not import the library.

The sums over the edges (21 of H, 6 of b, the robust chi2) are taken in one of three orders -- "asc" (edge order), "desc", "pair"
(pairwise tree) -- so that a test can measure how much of a result is summation noise.

optimize(obs, cam, Tcw, order) -> dict:
  n_corr, rounds, n_bad[4], iterations[4], chi2[4] (the active robust chi2 each round ended with), ret (the reference's return value),
  pose (3 x 4 double, the final [R | t]), Tcw (4 x 4 float32: Converter::toCvMat), outlier[n] (uint8; 0 where no point),
  flags[rounds][n_corr], margin[rounds][n_corr] = |chi2 - threshold| / threshold of every edge at each classification,
  class_chi2[rounds][n_corr] (the chi2 each classification used), idx[n_corr] (feature index of each edge), stale_used (a round ended on a rejected trial: active edges were classified at that pose),
  decisions: one (round, iteration, trial, accepted, currentChi, tempChi, max |x_j|) per damping trial,
  quat_flips: how often SE3Quat::normalizeRotation met w < 0, by call site (count_flips),
  stops: one (round, iteration, iniChi, currentChi) per evaluation of the added stop rule

path_sensitivity(res) -> the largest step max |x_j| among the trials whose accept / reject decision hangs on rounding (|currentChi - tempChi|
  <= NOISE max(currentChi, 1)), and the smallest relative distance of a stop-rule evaluation from its threshold.  A scene whose every
  noise-decided trial moves the pose by less than the comparison bound gives the same pose whichever way those decisions fall.
"""
import contextlib
import math

import numpy as np

f32 = np.float32
DELTA_MONO = float(f32(math.sqrt(5.991)))      # src/Optimizer.cc:322-323: const float
DELTA_STEREO = float(f32(math.sqrt(7.815)))
THR_MONO = f32(5.991)                          # :428-429
THR_STEREO = f32(7.815)
DBL_MAX = np.finfo(np.float64).max
NOISE = 1e-12                                  # path_sensitivity: a chi2 difference below NOISE * max(chi2, 1) is decided by rounding


# ---------------------------------------------------------------- SE3Quat: q = (x, y, z, w), t

QUAT_MUTATIONS = ("quat_branch1", "quat_branch2", "quat_branch3", "quat_tie_ge", "quat_no_flip")
_quat = dict(mutation=None, flips=dict(input=0, exp=0, mul=0, other=0))


@contextlib.contextmanager
def quat_mutation(name):
    """one deliberate error in the quaternion code below, for every model that uses it, while the block runs:
      "quat_branch1" / 2 / 3   in the branch of quat_from_matrix whose largest diagonal entry is 0 / 1 / 2, one off-diagonal sum is a difference
      "quat_tie_ge"            >= in the two comparisons of the diagonal entries
      "quat_no_flip"           quat_normalize does not flip the sign where w < 0"""
    assert name is None or name in QUAT_MUTATIONS, name
    before, _quat["mutation"] = _quat["mutation"], name
    try:
        yield
    finally:
        _quat["mutation"] = before


def count_flips():
    """-> a fresh counter dict that quat_normalize fills from now on: how often w < 0 made it flip, by call site ("input": pose_from_Tcw,
    "exp": se3_exp, "mul": pose_mul, "other").  The optimize() of each model puts it into its result as quat_flips."""
    _quat["flips"] = dict(input=0, exp=0, mul=0, other=0)
    return _quat["flips"]


def quat_from_matrix(m):
    """Eigen's Quaternion(Matrix3)"""
    mut = _quat["mutation"]
    t = (m[0, 0] + m[1, 1]) + m[2, 2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t, w])
    i = 0
    if m[1, 1] > m[0, 0] or (mut == "quat_tie_ge" and m[1, 1] == m[0, 0]):
        i = 1
    if m[2, 2] > m[i, i] or (mut == "quat_tie_ge" and m[2, 2] == m[i, i]):
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + 1.0)
    q = np.zeros(4)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[k, j] - m[j, k]) * t
    q[j] = (m[j, i] + m[i, j]) * t
    q[k] = (m[k, i] + m[i, k]) * t
    if mut == "quat_branch%d" % (i + 1):       # the sum that does not hold m01, which a look-at rotation with y down has as an exact zero
        if i == 0:
            q[k] = (m[k, i] - m[i, k]) * t
        else:
            q[j] = (m[j, i] - m[i, j]) * t
    return q


def quat_normalize(q, where="other"):
    """SE3Quat::normalizeRotation; `where` names the call site for count_flips()"""
    if q[3] < 0.0:
        _quat["flips"][where] += 1
        if _quat["mutation"] != "quat_no_flip":
            q = -q
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def quat_to_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def quat_rotate(q, v):
    """Eigen's Quaternion * vector; v is [..., 3]"""
    x, y, z, w = q
    X, Y, Z = v[..., 0], v[..., 1], v[..., 2]
    ux, uy, uz = 2.0 * (y * Z - z * Y), 2.0 * (z * X - x * Z), 2.0 * (x * Y - y * X)
    return np.stack([(X + w * ux) + (y * uz - z * uy), (Y + w * uy) + (z * ux - x * uz), (Z + w * uz) + (x * uy - y * ux)], axis=-1)


def pose_from_Tcw(Tcw):
    """Converter::toSE3Quat: the float matrix widened, SE3Quat(R, t)"""
    T = np.asarray(Tcw, f32).reshape(4, 4).astype(np.float64)
    return quat_normalize(quat_from_matrix(T[:3, :3]), "input"), T[:3, 3].copy()


def se3_exp(x):
    """SE3Quat::exp: x[0:3] rotation, x[3:6] translation -> (q, t)"""
    o = x[:3]
    theta = math.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    O = np.array([[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]])
    O2 = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            O2[r, c] = (O[r, 0] * O[0, c] + O[r, 1] * O[1, c]) + O[r, 2] * O[2, c]
    I = np.eye(3)
    if theta < 0.00001:
        R = (I + O) + O2
        V = R
    else:
        s, c = math.sin(theta), math.cos(theta)
        a, b, cc = s / theta, (1.0 - c) / (theta * theta), (theta - s) / ((theta * theta) * theta)
        R = (I + a * O) + b * O2
        V = (I + b * O) + cc * O2
    u = x[3:]
    t = np.array([(V[r, 0] * u[0] + V[r, 1] * u[1]) + V[r, 2] * u[2] for r in range(3)])
    return quat_normalize(quat_from_matrix(R), "exp"), t


def pose_mul(a, b):
    """SE3Quat::operator*"""
    (aq, at), (bq, bt) = a, b
    t = at + quat_rotate(aq, bt)
    ax, ay, az, aw = aq
    bx, by, bz, bw = bq
    q = np.array([((aw * bx + ax * bw) + ay * bz) - az * by,
                  ((aw * by + ay * bw) + az * bx) - ax * bz,
                  ((aw * bz + az * bw) + ax * by) - ay * bx,
                  ((aw * bw - ax * bx) - ay * by) - az * bz])
    return quat_normalize(q, "mul"), t


def oplus(pose, x):
    """VertexSE3Expmap::oplusImpl"""
    return pose_mul(se3_exp(np.asarray(x, np.float64)), pose)


# ---------------------------------------------------------------- edges

class Edges:
    """the correspondences of a frame, in feature order, widened to double"""

    def __init__(self, obs, cam):
        has = np.asarray(obs["has_point"]).astype(bool)
        self.idx = np.nonzero(has)[0]
        g = lambda k: np.asarray(obs[k], f32)[self.idx].astype(np.float64)
        self.mx, self.my, self.mr, self.w = g("x"), g("y"), g("u_right"), g("inv_sigma2")
        self.stereo = ~(np.asarray(obs["u_right"], f32)[self.idx] < f32(0))
        self.Xw = np.asarray(obs["Xw"], f32).reshape(-1, 3)[self.idx].astype(np.float64)
        self.fx, self.fy, self.cx, self.cy, self.bf = [float(v) for v in np.asarray(cam, f32)[:5]]
        self.n = len(self.idx)
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.thr = np.where(self.stereo, THR_STEREO, THR_MONO).astype(f32)

    def errors(self, pose):
        """-> Pc [n][3], err [n][3] (third row 0 for a monocular edge), chi2 [n]"""
        q, t = pose
        Pc = quat_rotate(q, self.Xw) + t
        x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
        with np.errstate(all="ignore"):
            invz_f = (1.0 / z).astype(f32).astype(np.float64)          # types_six_dof_expmap.cpp:300: a float
            us = (x * invz_f) * self.fx + self.cx
            vs = (y * invz_f) * self.fy + self.cy
            rs = us - self.bf * invz_f
            um = (x / z) * self.fx + self.cx
            vm = (y / z) * self.fy + self.cy
        e0 = self.mx - np.where(self.stereo, us, um)
        e1 = self.my - np.where(self.stereo, vs, vm)
        e2 = np.where(self.stereo, self.mr - rs, 0.0)
        chi_m = e0 * (self.w * e0) + e1 * (self.w * e1)
        chi_s = (e0 * (self.w * e0) + e1 * (self.w * e1)) + e2 * (self.w * e2)
        return Pc, np.stack([e0, e1, e2], axis=1), np.where(self.stereo, chi_s, chi_m)

    def jacobians(self, Pc):
        """types_six_dof_expmap.cpp:266-288 / :335-364 -> [n][3][6] (third row 0 for a monocular edge)"""
        x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
        fx, fy, bf = self.fx, self.fy, self.bf
        invz = 1.0 / z
        invz_2 = invz * invz
        A = np.zeros((self.n, 3, 6))
        A[:, 0, 0] = x * y * invz_2 * fx
        A[:, 0, 1] = -(1.0 + (x * x * invz_2)) * fx
        A[:, 0, 2] = y * invz * fx
        A[:, 0, 3] = -invz * fx
        A[:, 0, 5] = x * invz_2 * fx
        A[:, 1, 0] = (1.0 + y * y * invz_2) * fy
        A[:, 1, 1] = -x * y * invz_2 * fy
        A[:, 1, 2] = -x * invz * fy
        A[:, 1, 4] = -invz * fy
        A[:, 1, 5] = y * invz_2 * fy
        A[:, 2, 0] = A[:, 0, 0] - bf * y * invz_2
        A[:, 2, 1] = A[:, 0, 1] + bf * x * invz_2
        A[:, 2, 2] = A[:, 0, 2]
        A[:, 2, 3] = A[:, 0, 3]
        A[:, 2, 5] = A[:, 0, 5] - bf * invz_2
        A[~self.stereo, 2, :] = 0.0
        return A


def huber(chi2, delta):
    """RobustKernelHuber::robustify -> rho0, rho1"""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        out0 = 2.0 * sq * delta - dsqr
        out1 = delta / sq
    inl = chi2 <= dsqr
    return np.where(inl, chi2, out0), np.where(inl, 1.0, out1)


def ordered_sum(v, order):
    """sum over axis 0 of v [m, ...] in the named order, every addition rounded to double"""
    m = len(v)
    if m == 0:
        return np.zeros(v.shape[1:])
    if order == "asc" or order == "desc":
        seq = v if order == "asc" else v[::-1]
        acc = np.zeros(v.shape[1:])
        for k in range(m):
            acc = acc + seq[k]
        return acc
    if order == "pair":
        cur = v
        while len(cur) > 1:
            if len(cur) % 2:
                cur = np.concatenate([cur, np.zeros((1,) + cur.shape[1:])])
            cur = cur[0::2] + cur[1::2]
        return cur[0]
    raise ValueError(order)


def solve6(H, b, lam):
    """(H + lam I) x = b by LDL^T without pivoting -> x, or None unless every pivot is > 0"""
    A = H + lam * np.eye(6)
    L = np.zeros((6, 6))
    d = np.zeros(6)
    for j in range(6):
        dj = A[j, j]
        for m in range(j):
            dj -= (L[j, m] * L[j, m]) * d[m]
        if not dj > 0.0:
            return None
        d[j] = dj
        for i in range(j + 1, 6):
            v = A[i, j]
            for m in range(j):
                v -= (L[i, m] * L[j, m]) * d[m]
            L[i, j] = v / dj
    y = np.zeros(6)
    for i in range(6):
        v = b[i]
        for m in range(i):
            v -= L[i, m] * y[m]
        y[i] = v
    y = y / d
    x = np.zeros(6)
    for i in range(5, -1, -1):
        v = y[i]
        for m in range(i + 1, 6):
            v -= L[m, i] * x[m]
        x[i] = v
    return x


def build_system(E, pose, active, robust, order):
    """computeActiveErrors + buildSystem at pose -> H [6][6], b [6], the active robust chi2"""
    Pc, err, chi2 = E.errors(pose)
    A = E.jacobians(Pc)
    rho0, rho1 = huber(chi2, E.delta) if robust else (chi2, np.ones(E.n))
    rw = rho1 * E.w
    we = E.w[:, None] * err
    terms = np.zeros((E.n, 28))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            hm = (A[:, 0, r] * rw) * A[:, 0, c] + (A[:, 1, r] * rw) * A[:, 1, c]
            hs = hm + (A[:, 2, r] * rw) * A[:, 2, c]
            terms[:, k] = np.where(E.stereo, hs, hm)
            k += 1
        bm = A[:, 0, r] * we[:, 0] + A[:, 1, r] * we[:, 1]
        bs = bm + A[:, 2, r] * we[:, 2]
        terms[:, 21 + r] = -(rho1 * np.where(E.stereo, bs, bm))
    terms[:, 27] = rho0
    s = ordered_sum(terms[active], order)
    H = np.zeros((6, 6))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            H[r, c] = H[c, r] = s[k]
            k += 1
    return H, s[21:27].copy(), float(s[27])


def robust_chi2(E, pose, active, robust, order):
    _, _, chi2 = E.errors(pose)
    rho0 = huber(chi2, E.delta)[0] if robust else chi2
    return float(ordered_sum(rho0[active], order)), chi2


def optimize(obs, cam, Tcw, order="asc", hook=None):
    """hook(it, iteration, trial, accepted, pose): called after every trial (tests watch the Levenberg loop through it)"""
    E = Edges(obs, cam)
    n = len(np.asarray(obs["has_point"]))
    Tin = np.asarray(Tcw, f32).reshape(4, 4)
    res = dict(n_corr=E.n, rounds=0, n_bad=[0] * 4, iterations=[0] * 4, chi2=[0.0] * 4, ret=0, idx=E.idx, flags=[], margin=[],
               outlier=np.zeros(n, np.uint8), stale_used=False, decisions=[], stops=[], class_chi2=[], quat_flips=count_flips())
    if E.n < 3:                                                           # src/Optimizer.cc:423-424
        res["pose"] = Tin[:3, :].astype(np.float64)
        res["Tcw"] = Tin.copy()
        res["quat_flips"] = dict(res["quat_flips"])
        return res
    start = pose_from_Tcw(Tin)
    out = np.zeros(E.n, bool)
    pose = start
    x = np.zeros(6)
    for it in range(4):
        robust = it < 3
        pose = start                                                      # :437
        active = ~out
        trial_pose = start
        trial_chi2 = None
        lam, ni, stop_bad, iters = 0.0, 2.0, 0, 0
        cur = 0.0
        last_rejected = False
        for iteration in range(10):
            H, b, cur = build_system(E, pose, active, robust, order)
            ini = cur
            if iteration == 0:
                lam, ni, stop_bad = 1e-5 * max(0.0, *[abs(H[j, j]) for j in range(6)]), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                backup = pose
                sol = solve6(H, b, lam)
                if sol is not None:
                    x = sol
                pose = oplus(pose, x)
                trial_pose = pose
                temp, trial_chi2 = robust_chi2(E, pose, active, robust, order)
                if sol is None:
                    temp = DBL_MAX
                scale = 0.0
                for j in range(6):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                with np.errstate(all="ignore"):
                    rho = float((np.float64(cur) - np.float64(temp)) / np.float64(scale))
                accepted = rho > 0.0 and math.isfinite(temp)
                res["decisions"].append((it, iteration, qmax, accepted, cur, temp, float(np.abs(x).max())))
                if accepted:
                    t = 2.0 * rho - 1.0
                    alpha = min(1.0 - (t * t) * t, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur = temp
                else:
                    lam *= ni
                    ni *= 2.0
                    pose = backup                                         # pop(): the vertex only
                last_rejected = not accepted
                qmax += 1
                if hook:
                    hook(it, iteration, qmax - 1, accepted, trial_pose)
                if not (rho < 0.0 and qmax < 10):
                    break
            iters += 1
            if qmax == 10 or rho == 0.0:
                break
            res["stops"].append((it, iteration, ini, cur))
            stop_bad = stop_bad + 1 if (ini - cur) * 1e3 < ini else 0
            if stop_bad >= 3:
                break
        # :441-502
        _, _, fresh = E.errors(pose)
        chi2 = np.where(out, fresh, trial_chi2)
        res["stale_used"] = res["stale_used"] or (last_rejected and bool(active.any()))
        out = chi2.astype(f32) > E.thr
        res["class_chi2"].append(chi2.copy())
        res["flags"].append(out.copy())
        res["margin"].append(np.abs(chi2 - E.thr.astype(np.float64)) / E.thr.astype(np.float64))
        res["n_bad"][it] = int(out.sum())
        res["iterations"][it] = iters
        res["chi2"][it] = cur
        res["rounds"] = it + 1
        if E.n < 10:                                                      # :501
            break
    R = quat_to_matrix(pose[0])
    P = np.concatenate([R, pose[1][:, None]], axis=1)
    T = np.eye(4, dtype=f32)
    T[:3, :] = P.astype(f32)                                              # Converter::toCvMat(SE3Quat)
    res["pose"], res["Tcw"] = P, T
    res["outlier"][E.idx] = out
    res["ret"] = E.n - res["n_bad"][res["rounds"] - 1]
    res["quat_flips"] = dict(res["quat_flips"])                           # the counter stops here
    return res


def path_sensitivity(res):
    step = 0.0
    for (_, _, _, _, cur, temp, xmax) in res["decisions"]:
        if not math.isfinite(temp) or abs(cur - temp) <= NOISE * max(cur, 1.0):
            step = max(step, xmax)
    stop = 1.0
    for (_, _, ini, cur) in res["stops"]:
        if ini > 0.0:
            stop = min(stop, abs((ini - cur) * 1e3 - ini) / ini)
    return step, stop


def same_path(results):
    """results: optimize() of one scene in several summation orders -> whether they made the same accept / reject decisions, trial by trial"""
    a = [d[:4] for d in results[0]["decisions"]]
    return all([d[:4] for d in r["decisions"]] == a for r in results[1:])
