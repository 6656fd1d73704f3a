"""numpy float64 restatement of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:885-1153) with the pieces of g2o it runs:
g2o::Sim3 with its logarithm (Thirdparty/g2o/g2o/types/sim3.h), VertexSim3Expmap and EdgeSim3 (types_seven_dof_expmap.h:60-114), the numeric
BaseBinaryEdge::linearizeOplus and constructQuadraticForm (base_binary_edge.hpp:55-205), OptimizationAlgorithmLevenberg::solve with
setUserLambdaInit(1e-16) and SparseOptimizer::optimize.  Written from the reference text, independently of the kernels; one numpy operation
at a time, vectorised ACROSS EDGES and never inside an expression, so every operation is rounded on its own.  The exponential, the Sim3
product helpers' scalar forms and the ordered sums are tests/sim3opt_model.py's and tests/pose_model.py's.  It does not import the library.

optimize(problem, iterations, order, nudge, jacobian, mutation) -> dict.  problem is the dict orbx.optimize_essential_graph takes.

  variants (none of them an error; the spread between them is what a faithful implementation may differ by)
    order     "asc" | "desc" | "pair": the summation order of a vertex's blocks over its edges, of a pair's block over its edges, of chi2
              over the edges and of x (lambda x + b) over the vertices (pose_model.ordered_sum)
    nudge     None, or a seed: every sin, cos, exp, log and acos result is moved one ulp up or down by a seeded pattern; results every
              library gives exactly (sin 0, cos 0, exp 0, log 1, acos 1) are left alone
    jacobian  "numeric": the reference's central difference; "closed": the derivative it approximates, A = Jl^-1(e) Ad(C), B = -Jl^-1(e)
              Ad(C Si Sj^-1), Jl the left Jacobian of Sim3 summed from its series in the 7 x 7 adjoint

  mutations (each one a real error; tools/eg_spread.py --mutations measures what each moves)
    "lambda_diag"       lambda starts at 1e-5 x the largest diagonal entry instead of 1e-16
    "x6_not_zeroed"     oplusImpl does not zero update[6] under fix_scale (so the scale is optimised after all)
    "normal_from_vscw"  a normal edge measured from vScw where NonCorrectedSim3 holds the keyframe
    "normalise"         the quaternion normalised in Sim3's operator*
    "t_not_divided"     t not divided by s in the SE3 recovery
    "bta_untransposed"  a pair's block written untransposed where the row order asks for the transpose

  stage-level mutations (stages() alone takes them; tests/eg_stage_checks.py says which check of tests/test_eg_stages.py sees each)
    "g_sign"               b = +J^T e                          "plus_minus_swapped"   J = scalar (e(-delta) - e(+delta))
    "ij_blocks_swapped"    J = [B | A]                         "fixed_not_zeroed"     the columns of the fixed end kept
    "measurement_inverted" Siw * Swj for Sjw * Swi             "lambda_off_diagonal"  lambda on a diagonal block's whole lower triangle
    "y_not_b"              the right-hand side -b              "scale_without_lambda" a row's x (lambda x + b) without its lambda x
    "b_minus_one"          Sim3::log's B with the -1 the reference lacks in the branch (rotation < eps, scale >= eps): a repair, and
                           an error here, because the function restates the reference
    "lu_wrong_row"         with pivot row 2 of the 3 x 3 LU, the right-hand side's rows 1 and 2 exchanged instead of 0 and 2

stages(problem, lam, x, order, nudge, mutation) -> one linearisation and one trial, stage by stage, in the device's layout (see there).
The stages are module-level functions (measurements, xf_table, errors, jacobians, edge_products, rows_and_pairs, assemble, update,
vertex_scale) over a Graph; optimize() and stages() are both built from them.

Result: S [K][8], pose [K][3][4] (the double recovery [R | t / s]), point [P][3], n_free, iterations, trials, chi2_start, chi2, lambda,
lambda_init, branches[4] (how often Sim3::log took each branch, index 2 * (|sigma| >= eps) + (d <= 1 - eps), over every evaluation), decisions."""
import math

import numpy as np

import pose_model as pm
import sim3opt_model as sm

f32 = np.float32
DBL_MAX = pm.DBL_MAX
ORDERS = ("asc", "desc", "pair")
MUTATIONS = ("lambda_diag", "x6_not_zeroed", "normal_from_vscw", "normalise", "t_not_divided", "bta_untransposed")
STAGE_MUTATIONS = ("g_sign", "plus_minus_swapped", "ij_blocks_swapped", "fixed_not_zeroed", "measurement_inverted", "lambda_off_diagonal",
                   "y_not_b", "scale_without_lambda", "b_minus_one", "lu_wrong_row")
DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
EPS = 0.00001


class Libm(sm.Libm):
    """sim3opt_model's sin, cos, exp on scalars, and log, acos, sin, cos on arrays; with a seed each result one ulp up or down"""

    def _na(self, v, exact):
        if self.rng is None:
            return v
        up = self.rng.integers(0, 2, size=v.shape) == 1
        return np.where(exact, v, np.nextafter(v, np.where(up, np.inf, -np.inf)))

    def log_a(self, x):
        with np.errstate(all="ignore"):
            return self._na(np.log(x), x == 1.0)

    def acos_a(self, x):
        with np.errstate(all="ignore"):
            return self._na(np.arccos(x), x == 1.0)

    def sin_a(self, x):
        return self._na(np.sin(x), x == 0.0)

    def cos_a(self, x):
        return self._na(np.cos(x), x == 0.0)


# ---------------------------------------------------------------- g2o::Sim3 on arrays [n][8]: qx qy qz qw tx ty tz s, q never normalised

def qrot(q, v):
    """Eigen's Quaternion * vector, q [n][4], v [n][3]"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    ux = 2.0 * (y * Z - z * Y)
    uy = 2.0 * (z * X - x * Z)
    uz = 2.0 * (x * Y - y * X)
    return np.stack([(X + w * ux) + (y * uz - z * uy), (Y + w * uy) + (z * ux - x * uz), (Z + w * uz) + (x * uy - y * ux)], axis=1)


def mul(a, b, normalise=False):
    """sim3.h:266-272 on [n][8] (either side may be [1][8])"""
    n = max(len(a), len(b))
    a = np.broadcast_to(a, (n, 8))
    b = np.broadcast_to(b, (n, 8))
    ax, ay, az, aw = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    q = np.stack([((aw * bx + ax * bw) + ay * bz) - az * by,
                  ((aw * by + ay * bw) + az * bx) - ax * bz,
                  ((aw * bz + az * bw) + ax * by) - ay * bx,
                  ((aw * bw - ax * bx) - ay * by) - az * bz], axis=1)
    if normalise:
        q = np.where(q[:, 3:4] < 0.0, -q, q)
        nrm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        q = q / nrm[:, None]
    s = a[:, 7]
    t = s[:, None] * qrot(a[:, :4], b[:, 4:7]) + a[:, 4:7]
    return np.concatenate([q, t, (s * b[:, 7])[:, None]], axis=1)


def inverse(a):
    """sim3.h:233-236"""
    qc = np.stack([-a[:, 0], -a[:, 1], -a[:, 2], a[:, 3]], axis=1)
    k = -1.0 / a[:, 7]
    return np.concatenate([qc, qrot(qc, k[:, None] * a[:, 4:7]), (1.0 / a[:, 7])[:, None]], axis=1)


def smap(a, P):
    """sim3.h:144-146"""
    return a[:, 7:8] * qrot(a[:, :4], P) + a[:, 4:7]


def rot_matrix(q):
    """Eigen's toRotationMatrix of the quaternion as it stands -> [n][3][3]"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.zeros((len(q), 3, 3))
    R[:, 0, 0] = 1.0 - (tyy + tzz); R[:, 0, 1] = txy - twz; R[:, 0, 2] = txz + twy
    R[:, 1, 0] = txy + twz; R[:, 1, 1] = 1.0 - (txx + tzz); R[:, 1, 2] = tyz - twx
    R[:, 2, 0] = txz - twy; R[:, 2, 1] = tyz + twx; R[:, 2, 2] = 1.0 - (txx + tyy)
    return R


def lu3_solve(W, t, paths=None, wrong_row=False):
    """Eigen's 3 x 3 PartialPivLU and its solve on [n][3][3], [n][3]: the first row of the largest magnitude is the pivot, the entries below it
    divided by it, the trailing block updated entry by entry; forward with the unit lower triangle, backward with the upper one.
    paths: "pivot"[row] and "second"[exchanged] are counted up.  wrong_row (the mutation "lu_wrong_row"): with pivot row 2 the right-hand
    side has its rows 1 and 2 exchanged where the matrix has rows 0 and 2 (exchanging the wrong rows of BOTH is only another pivot order
    and the same solution)."""
    a = [[W[:, r, c].copy() for c in range(3)] for r in range(3)]
    b = [t[:, r].copy() for r in range(3)]

    def swap(cond, r1, r2, rhs=None):
        for c in range(3):
            a[r1][c], a[r2][c] = np.where(cond, a[r2][c], a[r1][c]), np.where(cond, a[r1][c], a[r2][c])
        r1, r2 = (r1, r2) if rhs is None else rhs
        b[r1], b[r2] = np.where(cond, b[r2], b[r1]), np.where(cond, b[r1], b[r2])

    with np.errstate(all="ignore"):
        big = np.abs(a[0][0])
        piv = np.zeros(len(t), int)
        m1 = np.abs(a[1][0]) > big
        big = np.where(m1, np.abs(a[1][0]), big); piv = np.where(m1, 1, piv)
        m2 = np.abs(a[2][0]) > big
        big = np.where(m2, np.abs(a[2][0]), big); piv = np.where(m2, 2, piv)
        swap(piv == 1, 0, 1)
        swap(piv == 2, 0, 2, (1, 2) if wrong_row else None)
        nz = big != 0.0
        a[1][0] = np.where(nz, a[1][0] / a[0][0], a[1][0]); a[2][0] = np.where(nz, a[2][0] / a[0][0], a[2][0])
        a[1][1] = a[1][1] - a[1][0] * a[0][1]; a[1][2] = a[1][2] - a[1][0] * a[0][2]
        a[2][1] = a[2][1] - a[2][0] * a[0][1]; a[2][2] = a[2][2] - a[2][0] * a[0][2]
        second = np.abs(a[2][1]) > np.abs(a[1][1])
        if paths is not None:
            for k in range(3):
                paths["pivot"][k] += int((piv == k).sum())
            paths["second"][0] += int((~second).sum()); paths["second"][1] += int(second.sum())
            paths.setdefault("rows", []).append((piv.copy(), second.copy()))
        swap(second, 1, 2)
        a[2][1] = np.where(a[1][1] != 0.0, a[2][1] / a[1][1], a[2][1])
        a[2][2] = a[2][2] - a[2][1] * a[1][2]
        y0 = b[0]
        y1 = b[1] - a[1][0] * y0
        y2 = b[2] - (a[2][0] * y0 + a[2][1] * y1)
        x2 = y2 / a[2][2]
        x1 = (y1 - a[1][2] * x2) / a[1][1]
        x0 = (y0 - (a[0][1] * x1 + a[0][2] * x2)) / a[0][0]
    return np.stack([x0, x1, x2], axis=1)


def skew(o):
    O = np.zeros((len(o), 3, 3))
    O[:, 0, 1] = -o[:, 2]; O[:, 0, 2] = o[:, 1]; O[:, 1, 2] = -o[:, 0]
    O[:, 1, 0] = o[:, 2]; O[:, 2, 0] = -o[:, 1]; O[:, 2, 1] = o[:, 0]
    return O


def log(S, lm, branches=None, paths=None, mutation=None):
    """sim3.h:148-230 on [n][8] -> [n][7].  paths["log_rows"] gets the branch index of every row of every call.  The mutation "b_minus_one"
    gives B of the branch with a rotation under eps and a scale above it the -1 the reference's text lacks (sim3.h:116, :199)"""
    t, s = S[:, 4:7], S[:, 7]
    sigma = lm.log_a(s)
    R = rot_matrix(S[:, :4])
    d = 0.5 * (((R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]) - 1.0)
    dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    ss = np.abs(sigma) < EPS
    sr = d > 1.0 - EPS
    if branches is not None:
        idx = np.where(ss, 0, 2) + np.where(sr, 0, 1)
        for k in range(4):
            branches[k] += int((idx == k).sum())
        if paths is not None:
            paths.setdefault("log_rows", []).append(idx.copy())
    with np.errstate(all="ignore"):
        dd = np.where(sr, 0.0, d)
        theta = lm.acos_a(dd)
        theta2 = theta * theta
        k = np.where(sr, 0.5, theta / (2.0 * np.sqrt(1.0 - dd * dd)))
        sigma2 = sigma * sigma
        C = np.where(ss, 1.0, (s - 1.0) / sigma)
        A01 = (1.0 - lm.cos_a(theta)) / theta2
        B01 = (theta - lm.sin_a(theta)) / (theta2 * theta)
        A10 = ((sigma - 1.0) * s + 1.0) / sigma2
        B10 = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
        if mutation == "b_minus_one":
            B10 = ((0.5 * sigma2 - sigma + 1.0) * s - 1.0) / (sigma2 * sigma)
        a = s * lm.sin_a(theta)
        b = s * lm.cos_a(theta)
        c = theta2 + sigma * sigma
        A11 = (a * sigma + (1.0 - b) * theta) / (theta * c)
        B11 = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2
    A = np.where(ss, np.where(sr, 1.0 / 2.0, A01), np.where(sr, A10, A11))
    B = np.where(ss, np.where(sr, 1.0 / 6.0, B01), np.where(sr, B10, B11))
    omega = k[:, None] * dR
    O = skew(omega)
    BO = B[:, None, None] * O
    W = np.zeros_like(O)
    for r in range(3):
        for cc in range(3):
            bo2 = (BO[:, r, 0] * O[:, 0, cc] + BO[:, r, 1] * O[:, 1, cc]) + BO[:, r, 2] * O[:, 2, cc]
            W[:, r, cc] = (A * O[:, r, cc] + bo2) + (C if r == cc else 0.0)
    ups = lu3_solve(W, t, paths, mutation == "lu_wrong_row")
    return np.concatenate([omega, ups, sigma[:, None]], axis=1)


def quat_branch(R):
    """which of the four branches Eigen's Quaternion(Matrix3) takes on R [3][3]: 0 the trace > 0, 1 + i the largest diagonal entry i"""
    if (R[0, 0] + R[1, 1]) + R[2, 2] > 0.0:
        return 0
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 1 + (2 if R[2, 2] > R[i, i] else i)


def exp_paths(u, paths):
    """counts the branch of Sim3(Vector7d) on u, 2 * (|sigma| >= eps) + (theta >= eps), and the branch of its Quaternion(R); R is
    restated here with the plain sin and cos, for the count alone"""
    u = np.asarray(u, np.float64)
    o = u[:3]
    theta = math.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    paths["exp"][(0 if abs(float(u[6])) < EPS else 2) + (0 if theta < EPS else 1)] += 1
    O = np.array([[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]])
    O2 = O @ O
    R = (np.eye(3) + O) + O2 if theta < EPS else (np.eye(3) + math.sin(theta) / theta * O) + (1.0 - math.cos(theta)) / (theta * theta) * O2
    paths["quat"][quat_branch(R)] += 1


def exp1(u, lm, paths=None):
    """Sim3(Vector7d) of one update -> [8]"""
    if paths is not None:
        exp_paths(u, paths)
    return sm.sim3_to8(sm.sim3_exp(np.asarray(u, np.float64), lm))


def vscw(problem, paths=None):
    """:923-937 -> [K][8]"""
    T = np.asarray(problem["Tcw"], f32).reshape(-1, 4, 4).astype(np.float64)
    cor = np.asarray(problem["corrected"]).reshape(-1)
    Sc = np.asarray(problem["S_corrected"], np.float64).reshape(-1, 8)
    V = np.zeros((len(T), 8))
    for k in range(len(T)):
        if cor[k] >= 0:
            V[k] = Sc[cor[k]]
        else:
            V[k, :4] = pm.quat_from_matrix(T[k, :3, :3]); V[k, 4:7] = T[k, :3, 3]; V[k, 7] = 1.0
            if paths is not None:
                paths["quat"][quat_branch(T[k, :3, :3])] += 1
    return V


def recover(S, divide=True):
    """:1108-1116 -> [K][3][4] double: [R | t * (1. / s)]"""
    R = rot_matrix(S[:, :4])
    inv = 1.0 / S[:, 7]
    t = S[:, 4:7] * inv[:, None] if divide else S[:, 4:7]
    return np.concatenate([R, t[:, :, None]], axis=2)


def correct_points(problem, V, S):
    """:1122-1152 -> [P][3] double"""
    X = np.asarray(problem["Xw"], f32).reshape(-1, 3).astype(np.float64)
    ref = np.asarray(problem["point_ref"]).reshape(-1).astype(int)
    if len(X) == 0:
        return np.zeros((0, 3))
    return smap(inverse(S[ref]), smap(V[ref], X))


# ---------------------------------------------------------------- the closed-form Jacobian's pieces

def adjoint(S):
    """Ad of [n][8] in g2o's order (omega, upsilon, sigma): exp(Ad u) = S exp(u) S^-1"""
    n = len(S)
    q = S[:, :4] / np.linalg.norm(S[:, :4], axis=1)[:, None]
    R = rot_matrix(q)
    t, s = S[:, 4:7], S[:, 7]
    Ad = np.zeros((n, 7, 7))
    Ad[:, :3, :3] = R
    Ad[:, 3:6, :3] = skew(t) @ R
    Ad[:, 3:6, 3:6] = s[:, None, None] * R
    Ad[:, 3:6, 6] = -t
    Ad[:, 6, 6] = 1.0
    return Ad


def jl_inverse(e):
    """the inverse of the left Jacobian of Sim3 at [n][7]: Jl = sum ad^k / (k + 1)!"""
    n = len(e)
    ad = np.zeros((n, 7, 7))
    ad[:, :3, :3] = skew(e[:, :3])
    ad[:, 3:6, :3] = skew(e[:, 3:6])
    ad[:, 3:6, 3:6] = skew(e[:, :3]) + e[:, 6, None, None] * np.eye(3)
    ad[:, 3:6, 6] = -e[:, 3:6]
    J = np.zeros((n, 7, 7))
    term = np.tile(np.eye(7), (n, 1, 1))
    for k in range(40):
        J = J + term
        term = term @ ad / (k + 2)
    return np.linalg.inv(J)


# ---------------------------------------------------------------- the solver

def solve_ldlt(H, b):
    """H x = b by LDL^T without pivoting (H's lower triangle) -> x, or None at a pivot that is not > 0.  THE STATED DEVIATION: g2o runs Eigen's
    sparse Cholesky on the same matrix, the library a dense LDL^T in another operation order; the same solution, other rounding."""
    n = len(b)
    L = np.zeros((n, n))
    d = np.zeros(n)
    for j in range(n):
        v = L[j, :j] * d[:j]
        dj = H[j, j] - L[j, :j] @ v
        if not dj > 0.0:
            return None
        d[j] = dj
        if j + 1 < n:
            L[j + 1:, j] = (H[j + 1:, j] - L[j + 1:, :j] @ v) / dj
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - L[i, :i] @ y[:i]
    y = y / d
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - L[i + 1:, i] @ x[i + 1:]
    return x


# ---------------------------------------------------------------- the stages, one function each; optimize() and stages() are built from them

def new_paths():
    """the path counters beside `branches`: the pivot row and the second exchange of lu3_solve, the four branches of the exponential
    (2 * (|sigma| >= eps) + (theta >= eps)) and of Quaternion(Matrix3) (0: trace > 0, 1 + i: diagonal entry i the largest)"""
    return dict(pivot=[0, 0, 0], second=[0, 0], exp=[0, 0, 0, 0], quat=[0, 0, 0, 0])


def measurements(problem, V, mutation=None):
    """:958-1092: Sji = Sjw * Swi -> [E][8]"""
    ei = np.asarray(problem["edge_i"]).reshape(-1).astype(int)
    ej = np.asarray(problem["edge_j"]).reshape(-1).astype(int)
    kind = np.asarray(problem["edge_kind"]).reshape(-1).astype(int)
    non = np.asarray(problem["noncorrected"]).reshape(-1)
    Snc = np.asarray(problem["S_noncorrected"], np.float64).reshape(-1, 8)

    def end(k, normal):
        use = normal & (non[k] >= 0) & (mutation != "normal_from_vscw")
        out = V[k].copy()
        out[use] = Snc[non[k][use]]
        return out
    if len(ei) == 0:
        return np.zeros((0, 8))
    if mutation == "measurement_inverted":
        return mul(end(ei, kind != 0), inverse(end(ej, kind != 0)))
    return mul(end(ej, kind != 0), inverse(end(ei, kind != 0)), mutation == "normalise")


def xf_table(fix, lm):
    """the 14 transforms Sim3(+-delta e_d) -> [14][8]: 2 d the plus side, 2 d + 1 the minus side"""
    xf = np.zeros((14, 8))
    for k in range(14):
        u = np.zeros(7)
        u[k // 2] = -DELTA if k & 1 else DELTA
        if fix:
            u[6] = 0.0
        xf[k] = exp1(u, lm)
    return xf


def chi2_of(err):
    c = err[:, 0] * err[:, 0]
    for m in range(1, 7):
        c = c + err[:, m] * err[:, m]
    return c


class Graph:
    """what a problem fixes before the first evaluation: the rows, the lists of a row's and a pair's edges, the start estimates, the
    measurements and the 14 transforms (in the order optimize() has always made them: the seeded nudges are drawn per call)"""

    def __init__(self, problem, lm, mutation=None, paths=None):
        self.lm, self.mutation, self.paths = lm, mutation, paths
        self.normalise = mutation == "normalise"
        fixed = np.asarray(problem["fixed"]).reshape(-1) != 0
        self.K = K = len(fixed)
        assert fixed.sum() == 1
        self.fix = bool(problem["fix_scale"]) and mutation != "x6_not_zeroed"
        self.ei = ei = np.asarray(problem["edge_i"]).reshape(-1).astype(int)
        self.ej = ej = np.asarray(problem["edge_j"]).reshape(-1).astype(int)
        self.E = E = len(ei)
        self.V = vscw(problem, paths)
        self.row = row = np.full(K, -1)
        row[~fixed] = np.arange(K - 1)
        self.F = F = K - 1
        self.branches = [0, 0, 0, 0]
        self.C = measurements(problem, self.V, mutation)
        self.xf = xf_table(self.fix, lm)
        self.free_i, self.free_j = row[ei] >= 0, row[ej] >= 0
        self.inc = [[] for _ in range(F)]            # per row: (edge, end) in edge order
        self.pairs = {}                              # (hi row, lo row) -> [(edge, transposed)] in edge order
        for e in range(E):
            ri, rj = row[ei[e]], row[ej[e]]
            if ri >= 0:
                self.inc[ri].append((e, 0))
            if rj >= 0:
                self.inc[rj].append((e, 1))
            if ri >= 0 and rj >= 0:
                self.pairs.setdefault((max(ri, rj), min(ri, rj)), []).append((e, ri < rj))


def errors(g, S, Si=None, Sj=None):
    """EdgeSim3::computeError of every edge -> [E][7]; Si / Sj: the ends' estimates where they are not S's"""
    Si = S[g.ei] if Si is None else Si
    Sj = S[g.ej] if Sj is None else Sj
    return log(mul(mul(g.C, Si, g.normalise), inverse(Sj), g.normalise), g.lm, g.branches, g.paths, g.mutation)


def jacobians(g, S, err, jacobian="numeric", evals=None):
    """[A | B] of every edge -> [E][7][14].  evals [E][29][7] gets the central difference's evaluations: 1 + 2 c the plus, 2 + 2 c the minus
    side of column c"""
    E = g.E
    A = np.zeros((E, 7, 14))
    if jacobian == "numeric":
        for c in range(14):
            on_i = c < 7
            d = c % 7
            plus = mul(g.xf[2 * d:2 * d + 1], S[g.ei] if on_i else S[g.ej], g.normalise)
            minus = mul(g.xf[2 * d + 1:2 * d + 2], S[g.ei] if on_i else S[g.ej], g.normalise)
            ep = errors(g, S, plus, None) if on_i else errors(g, S, None, plus)
            em = errors(g, S, minus, None) if on_i else errors(g, S, None, minus)
            if evals is not None:
                evals[:, 1 + 2 * c] = ep; evals[:, 2 + 2 * c] = em
            if g.mutation == "plus_minus_swapped":
                ep, em = em, ep
            A[:, :, c] = SCALAR * (ep - em)
    else:
        Ji = jl_inverse(err)
        E0 = mul(mul(g.C, S[g.ei]), inverse(S[g.ej]))
        A[:, :, :7] = Ji @ adjoint(g.C)
        A[:, :, 7:] = -(Ji @ adjoint(E0))
        if g.fix:
            A[:, :, 6] = 0.0
            A[:, :, 13] = 0.0
    if g.mutation == "ij_blocks_swapped":
        A = np.concatenate([A[:, :, 7:], A[:, :, :7]], axis=2)
    if g.mutation != "fixed_not_zeroed":
        A[~g.free_i, :, :7] = 0.0
        A[~g.free_j, :, 7:] = 0.0
    return A


def edge_products(g, err, J):
    """constructQuadraticForm's products of every edge: J^T J [E][14][14] (both triangles) and -J^T e [E][14], each entry the sum over
    the 7 error rows in ascending order"""
    E = g.E
    JtJ = np.zeros((E, 14, 14))
    for r in range(14):
        for c in range(r, 14):
            v = J[:, 0, r] * J[:, 0, c]
            for m in range(1, 7):
                v = v + J[:, m, r] * J[:, m, c]
            JtJ[:, r, c] = v
            JtJ[:, c, r] = v
    gv = np.zeros((E, 14))
    for c in range(14):
        e0 = err if g.mutation == "g_sign" else -err
        v = J[:, 0, c] * e0[:, 0]
        for m in range(1, 7):
            v = v + J[:, m, c] * e0[:, m]
        gv[:, c] = v
    return JtJ, gv


def rows_and_pairs(g, JtJ, gv, order):
    """the ordered sums: Hd [F][7][7], bv [F][7], the pair list [(hi row, lo row)] sorted, Off [NP][7][7] (dof of hi, dof of lo)"""
    F = g.F
    Hd, bv = np.zeros((F, 7, 7)), np.zeros((F, 7))
    for r in range(F):
        if not g.inc[r]:
            continue
        blocks = np.stack([JtJ[e, 7 * w:7 * w + 7, 7 * w:7 * w + 7] for e, w in g.inc[r]])
        Hd[r] = pm.ordered_sum(blocks, order)
        bv[r] = pm.ordered_sum(np.stack([gv[e, 7 * w:7 * w + 7] for e, w in g.inc[r]]), order)
    keys = sorted(g.pairs)
    Off = np.zeros((len(keys), 7, 7))
    for n, key in enumerate(keys):
        blocks = []
        for e, transposed in g.pairs[key]:
            AtB = JtJ[e, :7, 7:]
            blocks.append(AtB.T if (transposed and g.mutation != "bta_untransposed") else AtB)
        Off[n] = pm.ordered_sum(np.stack(blocks), order)
    return Hd, bv, keys, Off


def assemble(g, Hd, bv, keys, Off):
    """the symmetric H [n][n] and b [n] of the rows and pairs"""
    n = 7 * g.F
    H = np.zeros((n, n))
    for r in range(g.F):
        H[7 * r:7 * r + 7, 7 * r:7 * r + 7] = Hd[r]
    for (hi, lo), M in zip(keys, Off):
        H[7 * hi:7 * hi + 7, 7 * lo:7 * lo + 7] = M
        H[7 * lo:7 * lo + 7, 7 * hi:7 * hi + 7] = M.T
    return H, bv.reshape(-1).copy()


def update(g, S, x):
    """VertexSim3Expmap::oplusImpl of every row -> the trial estimates [K][8]"""
    T = S.copy()
    for k in range(g.K):
        if g.row[k] >= 0:
            T[k] = mul(exp1(x[7 * g.row[k]:7 * g.row[k] + 7], g.lm, g.paths)[None], S[k:k + 1], g.normalise)[0]
    return T


def vertex_scale(g, x, lam, b):
    """computeScale's part of every row: the sum over j ascending of x_j (lambda x_j + b_j) -> [F]"""
    per = np.zeros(g.F)
    for j in range(7):
        per = per + x[j::7] * ((b[j::7] if g.mutation == "scale_without_lambda" else lam * x[j::7] + b[j::7]))
    return per


def pack_upper(M):
    """the upper triangle of [..][N][N] in row order -> [..][N (N + 1) / 2]"""
    N = M.shape[-1]
    return np.stack([M[..., r, c] for r in range(N) for c in range(r, N)], axis=-1)


def stages(problem, lam, x=None, order="asc", nudge=None, mutation=None):
    """ONE linearisation at the start estimates and ONE trial from them with lambda = lam, as orbx_debug_eg_stages lays the device's
    stages out (include/orbx.h): vS, meas, xf, err [E][29][7] (the evaluations of a fixed end zeros), rec [E][120], echi, Hd [F][28], bv,
    pair [NP][2], Off [NP][49], status_lin, S [n][n] (lower triangle and diagonal, zeros above), y, x (given: the solve is skipped),
    solve_ok, trial [K][8], sc, echi_trial, status_trial; and branches, paths.  The sums behind status are taken in `order`."""
    assert mutation is None or mutation in MUTATIONS + STAGE_MUTATIONS
    lm = Libm(nudge)
    paths = new_paths()
    g = Graph(problem, lm, mutation, paths)
    E, F, K = g.E, g.F, g.K
    n = 7 * F
    S0 = g.V.copy()
    res = dict(vS=g.V, meas=g.C, xf=g.xf, n_pairs=0, branches=g.branches, paths=paths, graph=g)
    if E == 0 or F == 0:
        return res
    err = errors(g, S0)
    ev = np.zeros((E, 29, 7))
    ev[:, 0] = err
    J = jacobians(g, S0, err, "numeric", ev)
    ev[np.ix_(~g.free_i, 1 + np.arange(14))] = 0.0
    ev[np.ix_(~g.free_j, 15 + np.arange(14))] = 0.0
    chi = chi2_of(err)
    JtJ, gv = edge_products(g, err, J)
    Hd, bv, keys, Off = rows_and_pairs(g, JtJ, gv, order)
    H, b = assemble(g, Hd, bv, keys, Off)
    res.update(err=ev, rec=np.concatenate([pack_upper(JtJ), gv, chi[:, None]], axis=1), echi=chi, Hd=pack_upper(Hd), bv=bv,
               pair=np.array(keys, np.int32).reshape(-1, 2), n_pairs=len(keys), Off=Off.reshape(-1, 49),
               status_lin=np.array([float(pm.ordered_sum(chi, order)), 0.0, float(np.abs(np.diag(H)).max()), 0.0]))
    Sm = np.tril(H)
    if mutation == "lambda_off_diagonal":
        for r in range(F):
            blk = Sm[7 * r:7 * r + 7, 7 * r:7 * r + 7]
            blk[np.tril_indices(7)] += lam
    else:
        Sm[np.arange(n), np.arange(n)] += lam
    y = -b if mutation == "y_not_b" else b.copy()
    ok = -1
    if x is None:
        sol = solve_ldlt(H + lam * np.eye(n), b)
        ok = int(sol is not None)
        x = sol if sol is not None else np.zeros(n)
    else:
        x = np.array(x, np.float64).reshape(n)
    if g.fix:
        x[6::7] = 0.0
    T = update(g, S0, x)
    chi_t = chi2_of(errors(g, T))
    sc = vertex_scale(g, x, lam, b)
    res.update(S=Sm, y=y, x=x, solve_ok=ok, trial=T, sc=sc, echi_trial=chi_t,
               status_trial=np.array([float(pm.ordered_sum(chi_t, order)), float(pm.ordered_sum(sc, order)), res["status_lin"][2], float(ok == 1)]))
    return res


def optimize(problem, iterations=20, order="asc", nudge=None, jacobian="numeric", mutation=None):
    assert mutation is None or mutation in MUTATIONS
    lm = Libm(nudge)
    g = Graph(problem, lm, mutation)
    fix, E, F, V = g.fix, g.E, g.F, g.V

    def system(S):
        err = errors(g, S)
        chi = chi2_of(err)
        J = jacobians(g, S, err, jacobian)
        JtJ, gv = edge_products(g, err, J)
        H, b = assemble(g, *rows_and_pairs(g, JtJ, gv, order))
        return H, b, float(pm.ordered_sum(chi, order))

    S = V.copy()
    res = dict(n_free=F, iterations=0, trials=0, chi2_start=0.0, chi2=0.0, lambda_init=0.0, decisions=[])
    x = np.zeros(7 * F)
    lam, ni, stop_bad, cur = 0.0, 2.0, 0, 0.0
    for it in range(iterations if (E > 0 and F > 0) else 0):
        H, b, cur = system(S)
        ini = cur
        if it == 0:
            res["chi2_start"] = cur
            lam = 1e-5 * float(np.abs(np.diag(H)).max()) if mutation == "lambda_diag" else 1e-16
            ni, stop_bad = 2.0, 0
            res["lambda_init"] = lam
        rho, qmax = 0.0, 0
        while True:
            sol = solve_ldlt(H + lam * np.eye(7 * F), b)
            if sol is not None:
                x = sol
            if fix:
                x[6::7] = 0.0
            T = update(g, S, x)
            temp = float(pm.ordered_sum(chi2_of(errors(g, T)), order)) if sol is not None else DBL_MAX
            scale = float(pm.ordered_sum(vertex_scale(g, x, lam, b), order)) + 1e-3
            with np.errstate(all="ignore"):
                rho = float((np.float64(cur) - np.float64(temp)) / np.float64(scale))
            accepted = rho > 0.0 and math.isfinite(temp)
            res["decisions"].append((it, qmax, accepted, cur, temp))
            res["trials"] += 1
            if accepted:
                t = 2.0 * rho - 1.0
                alpha = min(1.0 - (t * t) * t, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = temp
                S = T
            else:
                lam *= ni
                ni *= 2.0
            qmax += 1
            if not (rho < 0.0 and qmax < 10):
                break
        res["iterations"] += 1
        if qmax == 10 or rho == 0.0:
            break
        with np.errstate(all="ignore"):
            stop_bad = stop_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if stop_bad >= 3:
            break
    res["chi2"] = cur
    res["lambda"] = lam
    res["S"] = S
    res["pose"] = recover(S, divide=mutation != "t_not_divided")
    res["point"] = correct_points(problem, V, S)
    res["vscw"] = V
    res["branches"] = g.branches
    return res
