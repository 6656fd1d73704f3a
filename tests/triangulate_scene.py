"""Two-view and stereo scenes for the triangulation tests, generated from a seed, and the suite the tests share.

A scene is a dict: k1 / k2s[i] = dict(x, y, octave, u_right, depth, raw_x, raw_y), v1 / v2s[i] = a view as tests/triangulate_model.py
takes it, pairs[n2][2*cap] int32 (-1 behind the lists), npairs[n2], cap, sf, sigma2, ratio_factor, name.
suite() builds every scene once, runs the model on it once (expected status, x3d, n_new per scene) and asserts that the suite covers every
status value of the contract, a failed earlier pair that does not block a later success, and a gate decided by the reference's :465 quirk."""
import functools

import numpy as np

import triangulate_model as tm

F = np.float32
NLEVELS = 8
SF = np.array([F(1.2) ** k for k in range(NLEVELS)], F)
SIGMA2 = (SF * SF).astype(F)
COUNTS = (0, 1, 63, 64, 65, 257)
N1 = 300
MIN_PARALLAX_COS = float(np.cos(np.deg2rad(1.0)))   # accepted triangulations have at least 1 degree between the rays


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def make_view(R, centre, fx=520.9, fy=521.0, cx=325.1, cy=249.7, mb=0.08):
    """the view of a camera with rotation R (world -> camera) at `centre`, as a keyframe keeps it: float Tcw, float Ow"""
    T = np.zeros((3, 4), F)
    T[:, :3] = R.astype(F)
    T[:, 3] = (-R @ centre).astype(F)
    fx, fy = F(fx), F(fy)
    return dict(Tcw=T, Ow=np.asarray(centre, F), fx=fx, fy=fy, cx=F(cx), cy=F(cy), invfx=F(1.0) / fx, invfy=F(1.0) / fy, mb=F(mb),
                mbf=F(mb) * fx)


def project(v, P):
    T = v["Tcw"].astype(np.float64)
    pc = P @ T[:, :3].T + T[:, 3]
    return float(v["fx"]) * pc[:, 0] / pc[:, 2] + float(v["cx"]), float(v["fy"]) * pc[:, 1] / pc[:, 2] + float(v["cy"]), pc[:, 2]


def make_keyframe(rng, v, P, octave, stereo_fraction, noise=0.3, raw_shift=False):
    u, w, z = project(v, P)
    n = len(P)
    x = (u + rng.normal(0, noise, n)).astype(F); y = (w + rng.normal(0, noise, n)).astype(F)
    stereo = (rng.random(n) < stereo_fraction) & (z > 0.1)
    ur = np.where(stereo, x - float(v["mbf"]) / np.where(stereo, z, 1.0) + rng.normal(0, 0.2, n), -1.0).astype(F)
    depth = np.where(stereo, z, -1.0).astype(F)
    k = dict(x=x, y=y, octave=octave.astype(np.int32), u_right=ur, depth=depth, raw_x=None, raw_y=None)
    if raw_shift:   # an unrectified camera: mvKeys differ from mvKeysUn by a smooth sub-pixel field
        k["raw_x"] = (x + F(0.4) * np.sin(y / F(50.0)).astype(F)).astype(F)
        k["raw_y"] = (y - F(0.3) * np.cos(x / F(70.0)).astype(F)).astype(F)
    return k


def make_scene(seed, counts, cap_extra=0, stereo1=0.0, stereo2=0.0, close=(), raw_shift=False, share=None, mbf2_scale=1.0, name=None):
    """counts[i] pairs for neighbour i; `close` names neighbours 5 mm away (no parallax: stereo depth or rejection); share = (i, j):
    neighbour j is neighbour i's keyframe and view again; mbf2_scale: the neighbours' baseline relative to keyframe 1's"""
    rng = np.random.default_rng(seed)
    n2 = len(counts)
    R1 = rodrigues(rng.normal(0, 0.02, 3)); c1 = rng.normal(0, 0.05, 3)
    v1 = make_view(R1, c1)
    # world points 2 to 8 m in front of camera 1, inside its image
    z = rng.uniform(2.0, 8.0, N1)
    px = rng.uniform(40, 600, N1); py = rng.uniform(40, 440, N1)
    pc = np.stack([(px - float(v1["cx"])) / float(v1["fx"]) * z, (py - float(v1["cy"])) / float(v1["fy"]) * z, z], 1)
    P = (pc - v1["Tcw"][:, 3].astype(np.float64)) @ v1["Tcw"][:, :3].astype(np.float64)
    oct1 = rng.integers(0, 3, N1)
    k1 = make_keyframe(rng, v1, P, oct1, stereo1, raw_shift=raw_shift)
    k2s, v2s, rows = [], [], []
    for i in range(n2):
        if share and i == share[1]:
            k2s.append(k2s[share[0]]); v2s.append(v2s[share[0]])
            perm = k2s[-1]["_perm"]
        else:
            ang = rng.uniform(0, 2 * np.pi)
            base = 0.005 if i in close else rng.uniform(0.35, 0.9)
            c2 = c1 + R1.T @ np.array([base * np.cos(ang), base * np.sin(ang), rng.normal(0, 0.02) if i not in close else 0.0])
            v2 = make_view(rodrigues(rng.normal(0, 0.03, 3)) @ R1, c2, mb=0.08 * mbf2_scale)
            perm = rng.permutation(N1)   # feature perm[p] of the neighbour sees point p
            inv = np.argsort(perm)
            oct2 = np.clip(oct1[inv] + rng.integers(-1, 2, N1), 0, NLEVELS - 1)
            k2 = make_keyframe(rng, v2, P[inv], oct2, stereo2, raw_shift=raw_shift)
            k2["_perm"] = perm
            k2s.append(k2); v2s.append(v2)
        idx1 = np.sort(rng.choice(N1, counts[i], replace=False))
        idx2 = perm[idx1].copy()
        wrong = rng.random(counts[i]) < 0.15           # a wrong match: another point's feature
        idx2[wrong] = rng.integers(0, N1, int(wrong.sum()))
        rows.append(np.stack([idx1, idx2], 1).reshape(-1))
    cap = max(max(counts), 1) + cap_extra
    pairs = np.full((n2, 2 * cap), -1, np.int32)
    for i, r in enumerate(rows):
        pairs[i, :len(r)] = r
    return dict(k1=k1, v1=v1, k2s=k2s, v2s=v2s, pairs=pairs, npairs=np.array(counts, np.int32), cap=cap, sf=SF, sigma2=SIGMA2,
                ratio_factor=F(1.5) * SF[1], name=name or f"seed{seed}")


def _one_pair_scene(name, k1, v1, k2, v2, pairs=((0, 0),)):
    pr = np.array(pairs, np.int32).reshape(1, -1)
    return dict(k1=k1, v1=v1, k2s=[k2], v2s=[v2], pairs=pr, npairs=np.array([len(pairs)], np.int32), cap=len(pairs), sf=SF, sigma2=SIGMA2,
                ratio_factor=F(1.5) * SF[1], name=name)


def _kf(x, y, octave=0, u_right=-1.0, depth=-1.0):
    a = lambda v, t: np.atleast_1d(np.asarray(v, t))
    return dict(x=a(x, F), y=a(y, F), octave=a(octave, np.int32), u_right=a(u_right, F), depth=a(depth, F), raw_x=None, raw_y=None)


def directed_scenes():
    """the statuses no random scene reaches reliably, each from one hand-made pair"""
    out = []
    I = np.eye(3)
    v1 = make_view(I, np.zeros(3))
    cx, cy, mbf = float(v1["cx"]), float(v1["cy"]), float(v1["mbf"])
    # 19: keyframe 1's stereo point at 2 m, parallel rays (no parallax: UnprojectStereo), the neighbour 3 m ahead of it
    ahead = make_view(I, np.array([0.0, 0.0, 3.0]))
    st = _kf(cx + 30, cy + 10, 0, cx + 30 - mbf / 2.0, 2.0)
    mono = _kf(cx + 30, cy + 10)
    out.append(_one_pair_scene("z2_behind", st, v1, mono, ahead))
    # 18: the mirror image: the neighbour's stereo point, keyframe 1 ahead of it
    out.append(_one_pair_scene("z1_behind", mono, ahead, st, v1))
    # 24: a stereo feature (u_right >= 0) whose depth is not positive reaches UnprojectStereo
    out.append(_one_pair_scene("no_depth", _kf(cx + 30, cy + 10, 0, cx + 25, -2.0), v1, mono, v1))
    # 17: w == 0 exactly.  No pair of rigid views gets there (the Jacobi leaves rounding in w), so the second "view" is degenerate: its
    # rotation block has a zero first row and its feature sits at cx, which makes row 2 of A (0, 0, 0, b) while column 3 is zero
    # elsewhere: the column is never rotated and is not the smallest.
    deg = make_view(I, np.array([0.5, 0.0, 0.0]))
    deg["Tcw"][0, :3] = 0
    out.append(_one_pair_scene("w_zero", _kf(cx + 150, cy + 40), v1, _kf(deg["cx"], cy + 41), deg))
    # 22: a zero distance.  With a view whose Ow belongs to its Tcw the depth test comes first, so Ow is set to the triangulated point.
    v2 = make_view(rodrigues(np.array([0.0, 0.02, 0.0])), np.array([0.6, 0.0, 0.0]))
    P = np.array([[0.4, -0.2, 4.0]])
    ka = _kf(*[c[0] for c in project(v1, P)[:2]]); kb = _kf(*[c[0] for c in project(v2, P)[:2]])
    st0, X = tm.test_pair(v1, ka, 0, v2, kb, 0, SF, SIGMA2, F(1.5) * SF[1])
    assert st0 == 0
    v2z = dict(v2, Ow=X.copy())
    out.append(_one_pair_scene("zero_distance", ka, v1, kb, v2z))
    # 23: the same pair with octaves three levels apart
    out.append(_one_pair_scene("scale_ratio", dict(ka, octave=np.array([0], np.int32)), v1, dict(kb, octave=np.array([5], np.int32)), v2))
    return out


def quirk_scene():
    """src/LocalMapping.cc:465 projects into the NEIGHBOUR's right image with the CURRENT keyframe's mbf.  Keyframe 1 is monocular here
    (its mbf enters nothing else), the neighbour is a stereo keyframe with twice the baseline: the gate of keyframe 2 passes with the
    neighbour's own mbf and fails with the one the reference uses."""
    v1 = make_view(np.eye(3), np.zeros(3))
    v2 = make_view(rodrigues(np.array([0.0, 0.02, 0.0])), np.array([0.6, 0.0, 0.0]), mb=0.16)
    P = np.array([[0.4, -0.2, 4.0]])
    u1, w1, _ = project(v1, P); u2, w2, z2 = project(v2, P)
    ka = _kf(u1[0], w1[0])
    kb = _kf(u2[0], w2[0], 0, u2[0] - float(v2["mbf"]) / z2[0], z2[0])
    s = _one_pair_scene("mbf_quirk", ka, v1, kb, v2)
    own = tm.test_pair(dict(v1, mbf=v2["mbf"]), ka, 0, v2, kb, 0, SF, SIGMA2, s["ratio_factor"])[0]
    ref = tm.test_pair(v1, ka, 0, v2, kb, 0, SF, SIGMA2, s["ratio_factor"])[0]
    assert (own, ref) == (0, tm.ST_REPROJ2), (own, ref)
    return s


def scenes():
    c = COUNTS
    out = []
    for k, n in enumerate(c):                                           # n2 = 1: every count, cap == count and cap larger
        out.append(make_scene(100 + k, (n,), cap_extra=(k % 2) * 7, stereo1=0.3 * (k % 2), stereo2=0.3 * (k // 3), name=f"one_{n}"))
    out.append(make_scene(1, (63, 64, 65), name="mono_mono"))          # n2 = 3: the four mixes
    out.append(make_scene(2, (257, 0, 1), stereo1=1.0, close=(2,), name="stereo_mono"))
    out.append(make_scene(3, (65, 63, 64), cap_extra=5, stereo2=1.0, close=(1,), name="mono_stereo"))
    out.append(make_scene(4, (64, 65, 63), stereo1=0.6, stereo2=0.6, close=(0, 2), name="stereo_stereo"))
    out.append(make_scene(5, (65, 64, 63), stereo1=0.5, stereo2=0.5, close=(1,), raw_shift=True, name="raw_positions"))
    out.append(make_scene(6, (64, 63, 65), stereo2=0.5, share=(0, 2), name="shared_frame"))
    out.append(make_scene(7, (63, 65, 64), stereo2=1.0, close=(0, 1, 2), name="close_stereo2"))
    out.append(make_scene(9, (64, 1, 0), cap_extra=1, stereo2=0.5, mbf2_scale=2.0, name="two_baselines"))
    out.append(make_scene(8, tuple(c[(3 * i + i // 6) % 6] for i in range(20)), cap_extra=3, stereo1=0.3, stereo2=0.3, close=(4, 11), name="twenty"))
    out += directed_scenes()
    out.append(quirk_scene())
    return out


@functools.lru_cache(maxsize=None)
def suite():
    """-> [(scene, (status, x3d, n_new))], computed once per process; the coverage the tests rely on is asserted here"""
    out = [(s, tm.first_wins(s)) for s in scenes()]
    seen = set()
    unblocked = False
    for s, (status, _x, _n) in out:
        failed_before = set()
        for i in range(len(s["k2s"])):
            row = status[i, :s["npairs"][i]]
            seen.update(int(v) for v in row)
            idx1 = s["pairs"][i, 0:2 * s["npairs"][i]:2]
            unblocked |= any(int(st) <= 2 and int(a) in failed_before for st, a in zip(row, idx1))
            failed_before.update(int(a) for st, a in zip(row, idx1) if 16 <= int(st) < 32)
        assert sum(s["npairs"]) % 256 != 0 or sum(s["npairs"]) == 0, s["name"]
    missing = set(tm.ALL_STATUS) - seen
    assert not missing, f"the suite reaches no status {sorted(missing)}"
    assert unblocked, "no failed pair is followed by a success of the same feature at a later neighbour"
    return out
