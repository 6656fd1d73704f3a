"""Synthetic loop closures for the OptimizeEssentialGraph tests (tests/test_eg_model.py, tests/test_essential_graph.py,
tests/test_eg_adapter.py, tools/eg_spread.py): what LoopClosing::CorrectLoop hands Optimizer::OptimizeEssentialGraph.

Keyframes stand on a closed path and look along it.  Their poses come from odometry that drifts in rotation, in translation and, when the
scale is free, in scale by 10 - 30 % over the loop.  Keyframe 0 is the loop keyframe (fixed), the last one the current keyframe; it and the
up to two keyframes in front of it carry a CorrectedSim3 (the current keyframe's from the loop measurement, the others' propagated through
their uncorrected relative pose, as :CorrectLoop does) and a NonCorrectedSim3 (their drifted pose at scale 1), and their float pose is the
corrected one.  Edges, in the order the function adds them: the LoopConnections edges (kind 0), then per keyframe in list order its
spanning-tree edge (some parents are not the predecessor), one earlier loop edge, and its covisibility edges that are neither of those nor in
sInsertedEdges (kind 1).  Map points hang on reference keyframes all over the list.

case(tag) -> (problem, options).  Tags: "<F>-free" / "<F>-fix" for F free keyframes, and the SPECIAL ones.
stage_case(name) -> the small designed inputs of the stage tests (STAGE_CASES, at the end of the file)."""
import math

import numpy as np

import eg_model as em
import pose_model as pm

f32 = np.float32
SIZES = (1, 4, 5, 9, 10, 37, 150)
BIG = 150
SPECIAL = ("two_edges_one_pair", "vertex_without_edge", "fixed_in_middle", "fixed_at_both_ends", "no_edges", "no_points", "half_radian",
           "no_iterations", "scale_only", "consistent-free", "consistent-fix", "stall-free")
# tools/eg_spread.py: seed shifts per tag (absent: 0); none was needed
SEED_SHIFT = {}


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _sim3(R, t, s):
    return np.concatenate([pm.quat_from_matrix(R), t, [s]])


def make(F, fix_scale, seed, rot_corr=None, scale_only=False, consistent=False, loop_edges=True, points=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    K = F + 1
    radius = 4.0 + rng.uniform(0, 2)
    # the true poses Tcw_k = [R | t]
    Rt, tt = [], []
    for k in range(K):
        a = 2 * math.pi * 0.97 * k / max(K - 1, 1) if K > 2 else 0.3 * k
        Rwc = _rot([0, 0, 1], a) @ _rot([1, 0, 0], 0.1 * math.sin(3 * a)) @ _rot([0, 1, 0], 0.05 * math.cos(2 * a))
        c = np.array([radius * math.cos(a), radius * math.sin(a), 0.3 * math.sin(2 * a)])
        Rt.append(Rwc.T); tt.append(-Rwc.T @ c)
    # drifting odometry: each relative motion with a small rotation and translation error and a scale step
    drift = 0.0 if (fix_scale or consistent) else rng.uniform(0.10, 0.30)
    step = (1.0 + drift) ** (1.0 / max(K - 1, 1))
    rot_noise = 0.0 if (consistent or scale_only) else 0.004
    tr_noise = 0.0 if (consistent or scale_only) else 0.01
    Rd, td = [Rt[0]], [tt[0]]
    run = 1.0
    for k in range(1, K):
        Rrel = Rt[k] @ Rt[k - 1].T
        trel = tt[k] - Rrel @ tt[k - 1]
        run *= step
        Rn = _rot(rng.normal(size=3), rot_noise * rng.uniform(0.5, 1.5)) if rot_noise else np.eye(3)
        Rrel = Rn @ Rrel
        trel = run * trel + tr_noise * rng.normal(size=3)
        Rd.append(Rrel @ Rd[k - 1]); td.append(Rrel @ td[k - 1] + trel)
    Tcw = np.zeros((K, 4, 4), f32)
    for k in range(K):
        Tcw[k, :3, :3] = Rd[k]; Tcw[k, :3, 3] = td[k]; Tcw[k, 3, 3] = 1
    cur = K - 1
    corrected = -np.ones(K, np.int32)
    noncorrected = -np.ones(K, np.int32)
    Sc, Sn = [], []
    if consistent:
        # every measurement agrees with the true poses: all keyframes carry them, as unit quaternions in double, in NonCorrectedSim3 (the
        # normal edges are measured from there), there is no LoopConnections edge, and the start estimates (CorrectedSim3) are off by a
        # Sim3 that grows along the path; the loop keyframe starts at its true pose.  consistent == "translation": off in translation only.
        # That matters with a free scale: where the rotation residual of an edge is under Sim3::log's eps while its scale residual is above
        # it, the reference's B = ((0.5 sigma^2 - sigma + 1) s) / sigma^3 (sim3.h:116, :199; the -1 of the series is missing) is of the order
        # 1 / sigma^3, the error is garbage and Levenberg rejects every step.  A start that is off in translation alone never enters that
        # branch and converges to rounding; the full offset stalls at chi2 = 8.6e-5 x the start (scene "stall-free", reported, not hidden).
        nbr = list(range(K))
        lm = em.Libm()
        for k in range(K):
            X = _sim3(Rt[k], tt[k], 1.0)
            X[:4] = X[:4] / np.linalg.norm(X[:4])
            w = k / max(K - 1, 1)
            u = w * np.array([0.03, -0.04, 0.05, 0.05, -0.03, 0.02, 0.0 if fix_scale else math.log(1.07)])
            if consistent == "translation":
                u[:3] = 0.0; u[6] = 0.0
            S = em.mul(em.exp1(u, lm)[None], X[None])[0]
            corrected[k] = len(Sc); noncorrected[k] = len(Sn)
            Sc.append(S); Sn.append(X)
            Tcw[k, :3, :] = em.recover(S[None])[0]
    else:
        nbr = [k for k in range(max(1, K - 3), K)]
        # NonCorrectedSim3: the drifted pose of the float matrix at scale 1; CorrectedSim3: the current keyframe from the loop, the others through it
        V0 = em.vscw(dict(Tcw=Tcw, corrected=-np.ones(K, np.int32), S_corrected=np.zeros((0, 8))))
        s_l = 1.0 if fix_scale else 1.0 / run
        Rc = Rt[cur] if rot_corr is None else _rot([0.3, -0.2, 1.0], rot_corr) @ Rd[cur]
        Rc = _rot(rng.normal(size=3), 0.001) @ Rc
        tc = s_l * (tt[cur] if rot_corr is None else td[cur]) + 0.005 * rng.normal(size=3)
        S_cur = _sim3(Rc, tc, s_l)
        for k in nbr:
            Sic = em.mul(V0[k:k + 1], em.inverse(V0[cur:cur + 1]))
            S = S_cur if k == cur else em.mul(Sic, S_cur[None])[0]
            corrected[k] = len(Sc); noncorrected[k] = len(Sn)
            Sc.append(S); Sn.append(V0[k].copy())
            Tcw[k, :3, :] = em.recover(S[None])[0]      # the corrected keyframe's pose is set before the call (CorrectLoop)
    Sc, Sn = np.array(Sc).reshape(-1, 8), np.array(Sn).reshape(-1, 8)
    fixed = np.zeros(K, np.uint8)
    fixed[0] = 1
    # edges
    ei, ej, kind = [], [], []
    inserted = set()
    if loop_edges and not consistent:
        loop_side = [k for k in range(0, min(3, K)) if k not in nbr]
        for a, i in enumerate(reversed(nbr)):
            for b, j in enumerate(loop_side):
                if a + b <= 2:
                    ei.append(i); ej.append(j); kind.append(0)
                    inserted.add((min(i, j), max(i, j)))
    parent = [-1] * K
    for k in range(1, K):
        parent[k] = k - 3 if (k >= 3 and k % 7 == 5) else k - 1
    loop_edge = {K // 2: 2} if K >= 12 else {}
    for k in range(K):
        if parent[k] >= 0:
            ei.append(k); ej.append(parent[k]); kind.append(1)
        if k in loop_edge:
            ei.append(k); ej.append(loop_edge[k]); kind.append(1)
        for kn in ([k - 2] + ([k - 3] if k % 3 == 0 else [])):
            if kn < 0 or kn == parent[k] or parent[kn] == k or loop_edge.get(k) == kn or (min(k, kn), max(k, kn)) in inserted:
                continue
            ei.append(k); ej.append(kn); kind.append(1)
    n_pts = 3 * K if points else 0
    ref = rng.integers(0, K, size=n_pts).astype(np.int32)
    if n_pts >= 2:
        ref[0] = 0; ref[1] = cur
    Xw = (rng.normal(size=(n_pts, 3)) * [radius, radius, 0.5]).astype(f32)
    return dict(Tcw=Tcw, fixed=fixed, corrected=corrected, noncorrected=noncorrected, S_corrected=Sc, S_noncorrected=Sn,
                edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), edge_kind=np.array(kind, np.uint8), Xw=Xw, point_ref=ref,
                fix_scale=int(bool(fix_scale)))


def permute(pr, order):
    """the keyframe list in another order: order[new] = old"""
    order = np.asarray(order)
    new_of = np.empty(len(order), np.int32)
    new_of[order] = np.arange(len(order), dtype=np.int32)
    out = dict(pr)
    for k in ("Tcw", "fixed", "corrected", "noncorrected"):
        out[k] = pr[k][order]
    out["edge_i"] = new_of[pr["edge_i"]]; out["edge_j"] = new_of[pr["edge_j"]]; out["point_ref"] = new_of[pr["point_ref"]]
    return out


def tag_of(F, fix):
    return f"{F}-{'fix' if fix else 'free'}"


def all_tags(big=True):
    return [tag_of(F, fix) for F in SIZES if big or F != BIG for fix in (0, 1)] + list(SPECIAL)


def case(tag, shift=None):
    """-> (problem, options)"""
    shift = SEED_SHIFT.get(tag, 0) if shift is None else shift
    opts = dict(iterations=20)
    for F in SIZES:
        for fix in (0, 1):
            if tag == tag_of(F, fix):
                return make(F, fix, 9100 + 2 * F + fix + 5000 * shift), opts
    seed = 9700 + SPECIAL.index(tag) + 5000 * shift
    if tag == "two_edges_one_pair":                 # a second and a third edge on the pair (6, 5), one of them the other way round
        pr = make(8, 0, seed)
        pr["edge_i"] = np.concatenate([pr["edge_i"], [6, 5]]).astype(np.int32); pr["edge_j"] = np.concatenate([pr["edge_j"], [5, 6]]).astype(np.int32)
        pr["edge_kind"] = np.concatenate([pr["edge_kind"], [1, 1]]).astype(np.uint8)
        return pr, opts
    if tag == "vertex_without_edge":                # keyframe 4 of 9 loses its edges; its neighbours stay connected through the covisibility edges
        pr = make(8, 1, seed)
        keep = (pr["edge_i"] != 4) & (pr["edge_j"] != 4)
        for k in ("edge_i", "edge_j", "edge_kind"):
            pr[k] = pr[k][keep]
        return pr, opts
    if tag == "fixed_in_middle":
        pr = make(9, 0, seed)
        return permute(pr, [1, 2, 3, 4, 0, 5, 6, 7, 8, 9]), opts
    if tag == "fixed_at_both_ends":                 # the loop keyframe as vertex 0 of one edge and as vertex 1 of others
        pr = make(6, 0, seed)
        pr["edge_i"] = np.concatenate([[0], pr["edge_i"]]).astype(np.int32); pr["edge_j"] = np.concatenate([[6], pr["edge_j"]]).astype(np.int32)
        pr["edge_kind"] = np.concatenate([[0], pr["edge_kind"]]).astype(np.uint8)
        return pr, opts
    if tag == "no_edges":
        pr = make(5, 0, seed)
        for k, t in (("edge_i", np.int32), ("edge_j", np.int32), ("edge_kind", np.uint8)):
            pr[k] = np.zeros(0, t)
        return pr, opts
    if tag == "no_points":
        return make(5, 1, seed, points=False), opts
    if tag == "half_radian":                        # a loop correction of about 0.5 rad: the acos branch at the start
        return make(12, 0, seed, rot_corr=0.5), opts
    if tag == "no_iterations":
        return make(7, 0, seed), dict(iterations=0)
    if tag == "scale_only":                         # drift in scale alone: rotation errors under the eps of Sim3::log next to scale errors above it
        return make(12, 0, seed, scale_only=True), opts
    if tag == "consistent-free":
        return make(12, 0, seed, consistent="translation"), opts
    if tag == "stall-free":
        return make(12, 0, seed, consistent=True), opts
    if tag == "consistent-fix":
        return make(12, 1, seed, consistent=True), opts
    raise KeyError(tag)


def consistent_truth(pr):
    """the one set of Sim3s a consistent scene's measurements agree with: NonCorrectedSim3 where there is one, else vScw"""
    V = em.vscw(pr)
    non = pr["noncorrected"]
    out = V.copy()
    out[non >= 0] = pr["S_noncorrected"][non[non >= 0]]
    return out


VARIANTS = [dict(order="asc"), dict(order="desc"), dict(order="pair"), dict(order="asc", nudge=1), dict(order="asc", nudge=2),
            dict(order="asc", jacobian="closed")]


def variants(pr, opts):
    """the model's answers across its variants, the plain one first.  The closed-form Jacobian is the derivative of the GROUP logarithm.  In
    the branch of Sim3::log with a rotation under eps and a scale above it (branches[2]) the reference's B lacks a -1 and its log is not the
    group's, so there the closed form is not the derivative of what the central difference differentiates: it is no variant of a scene
    whose plain run enters that branch, and is left out for it."""
    base = em.optimize(pr, **opts, **VARIANTS[0])
    rest = [v for v in VARIANTS[1:] if not (v.get("jacobian") == "closed" and base["branches"][2])]
    return [base] + [em.optimize(pr, **opts, **v) for v in rest]


# ---------------------------------------------------------------- the inputs of the stage tests (tests/test_eg_stages.py, tests/test_eg_stages_model.py)

THETA_EDGE = math.acos(1.0 - 1e-5)            # the rotation angle at which Sim3::log's d = 1 - eps
LOG_ANGLES = (0.0, 3e-6, THETA_EDGE - 1e-6, THETA_EDGE + 1e-6, 0.3, 3.0, 3.1)
LOG_AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 2, 3))
LOG_SIGMAS = (0.0, 3e-6, 1e-5 - 1e-9, 1e-5 + 1e-9, -(1e-5 - 1e-9), -(1e-5 + 1e-9), 0.2, -0.2)
STAGE_LAMBDA = 0.25                           # a lambda that no diagonal entry swallows in rounding, exact in binary
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float64)


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * math.sin(0.5 * angle), [math.cos(0.5 * angle)]]) if angle != 0.0 else np.array([0.0, 0.0, 0.0, 1.0])


def log_rows(fix_scale=1):
    """the designed start residuals (label, Sim3 [8]) of the log table: every angle x axis x scale, each with its own nonzero translation,
    then a row whose quaternion is -q and one whose quaternion has the norm 1 + 1e-3.  The four scales 1e-9 from eps are rows of the
    fix_scale table alone: with a free scale the central difference moves sigma by delta = 1e-9 itself, one of the two evaluations of
    columns 6 and 13 then has |sigma| = eps to the last bit, and which branch it takes is decided by the rounding of exp(1e-9) -- the
    model disagrees with itself there by 2e-6 across its nudges in every such row, so the rows would only test the last bit of exp."""
    rows = []
    n = 0
    for th in LOG_ANGLES:
        for ax in LOG_AXES:
            for sg in LOG_SIGMAS:
                if not fix_scale and abs(abs(sg) - 1e-5) < 1e-8:
                    continue
                t = np.array([0.3 + 0.07 * (n % 5), -0.2 + 0.11 * (n % 7), 0.5 - 0.13 * (n % 3)])
                t = np.roll(t, n % 3) * (-1.0 if n % 4 == 3 else 1.0)
                rows.append((f"theta {th:.9g} axis {ax} sigma {sg:.9g}", np.concatenate([_quat(ax, th), t, [math.exp(sg) if sg else 1.0]])))
                n += 1
    rows.append(("-q", np.concatenate([-_quat((1, 2, 3), 0.3), [0.4, -0.1, 0.2], [math.exp(0.2)]])))
    rows.append(("norm 1 + 1e-3", np.concatenate([(1.0 + 1e-3) * _quat((1, 2, 3), 0.3), [0.4, -0.1, 0.2], [math.exp(0.2)]])))
    return rows


def log_table(fix_scale=0):
    """one edge per designed residual D_r (log_rows): keyframe 0 is fixed and an identity, free keyframe 1 + r starts at S_corrected = D_r
    and is vertex 0 of edge r, whose vertex 1 is the fixed keyframe (r % 3 == 0) or the free identity keyframe FAR + r // 24.  All edges
    are normal edges and every keyframe's NonCorrectedSim3 is the identity, so every measurement is the identity exactly and the start
    error of edge r is log(D_r), the product with an identity being exact.  -> (problem, labels)"""
    rows = log_rows(fix_scale)
    R = len(rows)
    n_far = (R + 23) // 24
    K = 1 + R + n_far
    Tcw = np.tile(np.eye(4, dtype=f32), (K, 1, 1))
    fixed = np.zeros(K, np.uint8); fixed[0] = 1
    corrected = -np.ones(K, np.int32); corrected[1:1 + R] = np.arange(R)
    noncorrected = np.zeros(K, np.int32)
    Sc = np.array([d for _, d in rows])
    ei = 1 + np.arange(R, dtype=np.int32)
    ej = np.array([0 if r % 3 == 0 else 1 + R + r // 24 for r in range(R)], np.int32)
    return dict(Tcw=Tcw, fixed=fixed, corrected=corrected, noncorrected=noncorrected, S_corrected=Sc, S_noncorrected=IDENTITY[None].copy(),
                edge_i=ei, edge_j=ej, edge_kind=np.ones(R, np.uint8), Xw=np.zeros((0, 3), f32), point_ref=np.zeros(0, np.int32),
                fix_scale=int(bool(fix_scale))), [l for l, _ in rows]


EXP_OMEGAS = (("0", (0.0, 0.0, 0.0)), ("3e-6", (0.0, 3e-6, 0.0)), ("1e-5 - 1e-9", (1e-5 - 1e-9, 0.0, 0.0)), ("1e-5 + 1e-9", (0.0, 0.0, 1e-5 + 1e-9)),
              ("0.3", tuple(0.3 * np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0))), ("3.0 x", (3.0, 0.0, 0.0)), ("3.0 y", (0.0, 3.0, 0.0)),
              ("3.0 z", (0.0, 0.0, 3.0)))
EXP_SIGMAS = (0.0, 3e-6, 0.2, -0.2)


def _turned(k):
    """keyframe rotations for Quaternion(Matrix3): k % 4 == 0 the trace > 0, else a turn of 3 rad about axis k % 4 - 1 (that diagonal entry
    the largest, the trace below 0)"""
    return _rot([0.2, -0.1, 1.0], 0.4 + 0.1 * k) if k % 4 == 0 else _rot(np.eye(3)[k % 4 - 1] + 0.02 * np.array([1.0, -2.0, 1.5]), 3.0)


def chain(F, fix_scale, seed, fixed_at=0, extra=0):
    """F + 1 keyframes in a row joined by F spanning edges (keyframe k to k - 1, every third one written the other way round) and `extra`
    chords (k to k - 2).  The float poses turn through all four branches of Quaternion(Matrix3) (_turned); every fifth keyframe has a
    CorrectedSim3 with a scale of its own, every seventh a NonCorrectedSim3.  The edges alternate between the two kinds."""
    rng = np.random.Generator(np.random.PCG64(seed))
    K = F + 1
    Tcw = np.zeros((K, 4, 4), f32)
    Sc, Sn = [], []
    corrected, noncorrected = -np.ones(K, np.int32), -np.ones(K, np.int32)
    for k in range(K):
        R = _turned(k)
        t = np.array([0.5 * k, 0.3 * math.sin(k), 0.1 * k]) + 0.05 * rng.normal(size=3)
        Tcw[k, :3, :3] = R; Tcw[k, :3, 3] = t; Tcw[k, 3, 3] = 1
        if k % 5 == 4:
            corrected[k] = len(Sc)
            Sc.append(_sim3(_rot(rng.normal(size=3), 0.02) @ R, t + 0.02 * rng.normal(size=3), 1.0 if fix_scale else 1.0 + 0.1 * rng.uniform(-1, 1)))
        if k % 7 == 3:
            noncorrected[k] = len(Sn)
            Sn.append(_sim3(_rot(rng.normal(size=3), 0.01) @ R, t + 0.01 * rng.normal(size=3), 1.0))
    fixed = np.zeros(K, np.uint8); fixed[fixed_at] = 1
    ei, ej = [], []
    for k in range(1, K):
        a, b = (k, k - 1) if k % 3 else (k - 1, k)
        ei.append(a); ej.append(b)
    for n in range(extra):
        k = 2 + n % max(K - 2, 1)
        ei.append(k); ej.append(k - 2)
    E = len(ei)
    return dict(Tcw=Tcw, fixed=fixed, corrected=corrected, noncorrected=noncorrected, S_corrected=np.array(Sc).reshape(-1, 8),
                S_noncorrected=np.array(Sn).reshape(-1, 8), edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32),
                edge_kind=(np.arange(E) % 2).astype(np.uint8), Xw=np.zeros((0, 3), f32), point_ref=np.zeros(0, np.int32), fix_scale=int(bool(fix_scale)))


def exp_table(fix_scale):
    """a chain with one free keyframe per (omega, sigma) of EXP_OMEGAS x EXP_SIGMAS and the update x_in that holds them, each with a nonzero
    upsilon -> (problem, x_in [7 F], labels [F])"""
    labels, xs = [], []
    n = 0
    for name, om in EXP_OMEGAS:
        for sg in EXP_SIGMAS:
            ups = np.roll(np.array([0.05 + 0.01 * (n % 4), -0.03, 0.02 * (1 + n % 3)]), n % 3)
            xs.append(np.concatenate([om, ups, [sg]])); labels.append(f"omega {name} sigma {sg:.9g}")
            n += 1
    return chain(len(xs), fix_scale, 9900 + int(bool(fix_scale))), np.concatenate(xs), labels


SHAPES = ("edges-1", "edges-7", "edges-8", "edges-9", "edges-17", "fixed-is-i", "fixed-has-no-edge", "two_edges_one_pair", "vertex_without_edge",
          "fixed_in_middle", "fixed_at_both_ends")


def shape(tag):
    """the small graphs of the stage tests.  edges-E: E edges, so that k_eg_edges<true>'s workgroups of eight are a single slot, part
    filled, exactly full, full and one more, and two and one more; the fixed keyframe is vertex 1 of its edges (vertex 0 of both
    its edges in fixed-is-i, and of no edge in fixed-has-no-edge).  The named special
    scenes are case()'s.  The odd ones are fix_scale scenes."""
    if tag.startswith("edges-"):
        E = int(tag[6:])
        F = min(E, 5)
        return chain(F, E % 2, 9800 + E, extra=E - F)
    if tag == "fixed-is-i":
        return chain(6, 0, 9850, fixed_at=5, extra=3)
    if tag == "fixed-has-no-edge":
        pr = chain(6, 1, 9851, extra=4)
        pr2 = {k: (np.concatenate([v, v[:1]]) if k in ("Tcw", "fixed", "corrected", "noncorrected") else v) for k, v in pr.items()}
        pr2["fixed"] = pr2["fixed"].copy(); pr2["fixed"][:] = 0; pr2["fixed"][-1] = 1     # a copy of keyframe 0 behind the list, fixed, without an edge
        return pr2
    return case(tag)[0]


def long_chain(fix_scale=0):
    """260 free keyframes and 300 edges: more than one stride of 256 in k_eg_reduce's sums over the edges and the rows and in the update"""
    return chain(260, fix_scale, 9870, fixed_at=130, extra=40)


def long_chain_x(F=260):
    """an update for long_chain: small, every dof nonzero"""
    rng = np.random.Generator(np.random.PCG64(9871))
    return 0.01 * rng.normal(size=7 * F)


STAGE_CASES = ("log-free", "log-fix", "exp-free", "exp-fix", "long-free") + tuple("shape-" + t for t in SHAPES)
_stage_cache = {}


def stage_case(name):
    """-> dict(problem, lam, x (None: the device solves), labels (of the rows of err, or of trial for an exp table), S (whether the n x n
    matrix is worth dumping))"""
    if name.startswith("log-"):
        pr, labels = log_table(name == "log-fix")
        return dict(problem=pr, lam=STAGE_LAMBDA, x=None, labels=labels, S=False)
    if name.startswith("exp-"):
        pr, x, labels = exp_table(name == "exp-fix")
        return dict(problem=pr, lam=STAGE_LAMBDA, x=x, labels=["fixed"] + labels, S=True)
    if name == "long-free":
        pr = long_chain(0)
        return dict(problem=pr, lam=STAGE_LAMBDA, x=long_chain_x(), labels=[f"edge {e}" for e in range(len(pr["edge_i"]))], S=False)
    pr = shape(name[6:])
    return dict(problem=pr, lam=STAGE_LAMBDA, x=None, labels=[f"edge {e}" for e in range(len(pr["edge_i"]))], S=True)


def stage_models(name, mutation=None):
    """the model's stages of a case at the nudge settings None, 1, 2 (computed once), or under a mutation without a nudge"""
    key = (name, mutation)
    if key not in _stage_cache:
        c = stage_case(name)
        nudges = (None, 1, 2) if mutation is None else (None,)
        _stage_cache[key] = [em.stages(c["problem"], c["lam"], c["x"], nudge=n, mutation=mutation) for n in nudges]
    return _stage_cache[key]
