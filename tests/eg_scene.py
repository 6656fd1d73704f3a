"""Synthetic loop closures for the OptimizeEssentialGraph tests (tests/test_eg_model.py, tests/test_essential_graph.py,
tests/test_eg_adapter.py, tools/eg_spread.py): what LoopClosing::CorrectLoop hands Optimizer::OptimizeEssentialGraph.

Keyframes stand on a closed path and look along it.  Their poses come from odometry that drifts in rotation, in translation and, when the
scale is free, in scale by 10 - 30 % over the loop.  Keyframe 0 is the loop keyframe (fixed), the last one the current keyframe; it and the
up to two keyframes in front of it carry a CorrectedSim3 (the current keyframe's from the loop measurement, the others' propagated through
their uncorrected relative pose, as :CorrectLoop does) and a NonCorrectedSim3 (their drifted pose at scale 1), and their float pose is the
corrected one.  Edges, in the order the function adds them: the LoopConnections edges (kind 0), then per keyframe in list order its
spanning-tree edge (some parents are not the predecessor), one earlier loop edge, and its covisibility edges that are neither of those nor in
sInsertedEdges (kind 1).  Map points hang on reference keyframes all over the list.

case(tag) -> (problem, options).  Tags: "<F>-free" / "<F>-fix" for F free keyframes, and the SPECIAL ones."""
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
