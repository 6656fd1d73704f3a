"""The scenes of pose optimisation, local and global bundle adjustment in TURNED world frames, and a table of exact rotations: data and
helpers only.  tests/pose_scene.py draws its camera near the identity and tests/lba_scene.py looks at the origin from an arc of +-0.7 rad,
so every float Tcw of those scenes has a positive trace and Eigen's Quaternion(Matrix3) (quat_from_matrix of orbx_lm.h) takes its first
branch.  Turning the world by a rotation G,

    Tcw' = float32(Tcw . diag(G^T, 1)),   Xw' = float32(G . Xw),

keeps the geometry in the camera frame and puts the start rotations into the other three branches.  For the exact half turns (G a
diagonal of +-1) the turned problem is the same problem with sign flips of its inputs, bit for bit.

TURNS            the named world turns: x3 y3 z3 (3 rad about an axis: every pose lands in branch 1, 2, 3), d22 (2.2 rad about (1,1,1)/sqrt 3:
                 the keyframes of one problem spread over several branches), pix piy piz (the exact half turns)
POSE_CASES       (n_corr, mix, turn): 10 is the smallest size that runs all four rounds, 65 crosses a wave
LBA_CASES        (shape, mix, turn): the one-row shape and the smallest with several rows
GBA_CASES        (shape, turn): the first three of gba_scene.SHAPES, and the fourth (12 keyframes) under d22, where it is in all four branches
*_SEED_SHIFT     tools/turned_spread.py --select: per case the first of 32 seed shifts whose scene is admissible (absent: 0)
*_PAIR_SHIFT     the metamorphic test of a half turn runs the turned and the un-turned scene of one seed, and both have to be admissible:
                 where the un-turned scene of the case's own seed is not, the first shift at which both are (absent: the case's own)
EXACT_ROTATIONS  (name, float32 matrix, branch, sign of the raw w): eight exact matrices (two cyclic permutations with trace 0, the three half
                 turns with w = +0, three with two equal largest diagonal entries) and seeded rotations built from a quaternion whose
                 dominant component and sign of w are chosen, so that what each is expected to do does not come from the code under test."""
import math

import numpy as np

import gba_scene as gs
import lba_scene as ls
import pose_scene as ps

f32 = np.float32
HALF_TURNS = ("pix", "piy", "piz")
TURNS = {
    "x3": ps.rodrigues(np.array([3.0, 0.0, 0.0])),
    "y3": ps.rodrigues(np.array([0.0, 3.0, 0.0])),
    "z3": ps.rodrigues(np.array([0.0, 0.0, 3.0])),
    "d22": ps.rodrigues(2.2 * np.ones(3) / math.sqrt(3.0)),
    "pix": np.diag([1.0, -1.0, -1.0]),
    "piy": np.diag([-1.0, 1.0, -1.0]),
    "piz": np.diag([-1.0, -1.0, 1.0]),
}
TURN_BRANCH = dict(x3=1, y3=2, z3=3, pix=1, piy=2, piz=3)     # where these turns put every start pose of the scenes; d22 spreads them

POSE_SIZES = (10, 65)
LBA_SHAPES = ((1, 1, 8), (3, 2, 64))
GBA_SHAPES = tuple(gs.SHAPES[:3])
POSE_CASES = [(n, mix, turn) for n in POSE_SIZES for mix in ps.MIXES for turn in TURNS]
LBA_CASES = [(shape, mix, turn) for shape in LBA_SHAPES for mix in ls.MIXES for turn in TURNS]
# the first three shapes hold two or three keyframes, which d22 leaves in two branches: the smallest shape with more joins them under d22 alone
GBA_CASES = [(shape, turn) for shape in GBA_SHAPES for turn in TURNS] + [(gs.SHAPES[3], "d22")]

# python tools/turned_spread.py --select
POSE_SEED_SHIFT = {(10, 'mono', 'x3'): 6, (10, 'mono', 'y3'): 6, (10, 'mono', 'z3'): 6, (10, 'mono', 'd22'): 6, (10, 'mono', 'pix'): 6,
                   (10, 'mono', 'piy'): 6, (10, 'mono', 'piz'): 6, (10, 'mixed', 'd22'): 2, (10, 'mixed', 'piy'): 2, (10, 'mixed', 'piz'): 2,
                   (65, 'mono', 'y3'): 1, (65, 'mono', 'z3'): 2, (65, 'mono', 'd22'): 1, (65, 'mono', 'pix'): 5, (65, 'mono', 'piy'): 1,
                   (65, 'mono', 'piz'): 5, (65, 'mixed', 'z3'): 2, (65, 'mixed', 'd22'): 1}
LBA_SEED_SHIFT = {((1, 1, 8), 'mixed', 'x3'): 2, ((1, 1, 8), 'mixed', 'y3'): 2, ((1, 1, 8), 'mixed', 'z3'): 2, ((1, 1, 8), 'mixed', 'd22'): 2,
                  ((1, 1, 8), 'mixed', 'pix'): 2, ((1, 1, 8), 'mixed', 'piy'): 2, ((1, 1, 8), 'mixed', 'piz'): 2}
GBA_SEED_SHIFT = {((1, 60, 'mono', 20), 'x3'): 8, ((1, 60, 'mono', 20), 'y3'): 8, ((1, 60, 'mono', 20), 'z3'): 8, ((1, 60, 'mono', 20), 'd22'): 8,
                  ((1, 60, 'mono', 20), 'pix'): 8, ((1, 60, 'mono', 20), 'piy'): 8, ((1, 60, 'mono', 20), 'piz'): 8}
POSE_PAIR_SHIFT = {(10, 'mixed', 'pix'): 6, (10, 'mixed', 'piy'): 6, (10, 'mixed', 'piz'): 5, (65, 'mono', 'pix'): 38, (65, 'mono', 'piy'): 103,
                   (65, 'mono', 'piz'): 29}
LBA_PAIR_SHIFT = {}
GBA_PAIR_SHIFT = {}


def branch_of(R):
    """the branch of Eigen's Quaternion(Matrix3) on the float matrix widened to double: 0 the trace > 0, 1 + i the largest diagonal entry i
    (the later one only where it is strictly larger)"""
    R = np.asarray(R, f32).astype(np.float64)
    if (R[0, 0] + R[1, 1]) + R[2, 2] > 0.0:
        return 0
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 1 + (2 if R[2, 2] > R[i, i] else i)


def _turn_T(T, G):
    """[..., 4, 4] float32 -> float32(T . diag(G^T, 1))"""
    D = np.eye(4)
    D[:3, :3] = G.T
    return (np.asarray(T, f32).astype(np.float64) @ D).astype(f32)


def _turn_X(X, G):
    return (np.asarray(X, f32).astype(np.float64) @ G.T).astype(f32)


def turn_pose_scene(sc, G):
    """a pose_scene.scene in the world turned by G: the start pose, the true pose and the points; everything else as it is"""
    out = dict(sc)
    out["obs"] = dict(sc["obs"], Xw=_turn_X(sc["obs"]["Xw"], G))
    out["Tcw"] = _turn_T(sc["Tcw"], G)
    D = np.eye(4)
    D[:3, :3] = G.T
    out["Tcw_true"] = sc["Tcw_true"] @ D
    return out


def turn_problem(sc, G):
    """a scene of lba_scene / gba_scene in the world turned by G: the keyframes' Tcw, the points, the truth; everything else as it is"""
    out = dict(sc)
    pr = sc["problem"]
    out["problem"] = dict(pr, Tcw=_turn_T(pr["Tcw"], G), Xw=_turn_X(pr["Xw"], G))
    truth = sc["truth_pose"].copy()
    truth[:, :, :3] = truth[:, :, :3] @ G.T
    out["truth_pose"] = truth
    out["truth_X"] = sc["truth_X"] @ G.T
    return out


def turn_back_pose(pose, G):
    """[..., 3, 4] double: the rotation block times G (the inverse of what turn_* did to it), the translation as it is"""
    out = np.array(pose, np.float64)
    out[..., :3] = out[..., :3] @ G
    return out


def turn_back_points(X, G):
    return np.asarray(X, np.float64) @ G        # rows: (G^T x)^T = x^T G


def pose_case(n, mix, turn, shift=None):
    """-> the scene of POSE_CASES' (n, mix, turn); turn None with a shift: the un-turned scene of that seed"""
    shift = POSE_SEED_SHIFT.get((n, mix, turn), 0) if shift is None else shift
    sc = ps.scene(1000 * ps.MIXES.index(mix) + n + 5000 * shift, n, mix)
    return sc if turn is None else turn_pose_scene(sc, TURNS[turn])


def lba_case(shape, mix, turn, shift=None):
    shift = LBA_SEED_SHIFT.get((shape, mix, turn), 0) if shift is None else shift
    sc = ls.shape_scene(shape, mix, shift)
    return sc if turn is None else turn_problem(sc, TURNS[turn])


def gba_options(shape):
    return dict(iterations=shape[3], robust=True)


def gba_case(shape, turn, shift=None):
    """-> (scene, options for gba_model.optimize and bundle_adjustment alike)"""
    shift = GBA_SEED_SHIFT.get((shape, turn), 0) if shift is None else shift
    sc = gs.shape_scene(shape, shift)
    return (sc if turn is None else turn_problem(sc, TURNS[turn])), gba_options(shape)


def pose_pair(n, mix, turn):
    """-> (the turned scene, the un-turned scene of the same seed) of a half-turn case, at the shift where both are admissible"""
    shift = POSE_PAIR_SHIFT.get((n, mix, turn), POSE_SEED_SHIFT.get((n, mix, turn), 0))
    return pose_case(n, mix, turn, shift), pose_case(n, mix, None, shift)


def lba_pair(shape, mix, turn):
    shift = LBA_PAIR_SHIFT.get((shape, mix, turn), LBA_SEED_SHIFT.get((shape, mix, turn), 0))
    return lba_case(shape, mix, turn, shift), lba_case(shape, mix, None, shift)


def gba_pair(shape, turn):
    shift = GBA_PAIR_SHIFT.get((shape, turn), GBA_SEED_SHIFT.get((shape, turn), 0))
    return gba_case(shape, turn, shift)[0], gba_case(shape, None, shift)[0]


def pose_tag(n, mix, turn):
    return f"{n}-{mix}-{turn}"


def lba_tag(shape, mix, turn):
    return f"{shape[0]}-{shape[1]}-{shape[2]}-{mix}-{turn}"


def gba_tag(shape, turn):
    return f"{gs.tag_of(shape)}-{turn}"


def branches_of_problem(pr):
    return [branch_of(T[:3, :3]) for T in np.asarray(pr["Tcw"], f32).reshape(-1, 4, 4)]


# ---------------------------------------------------------------- exact rotations

def _from_quat(x, y, z, w):
    n = math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).astype(f32)


def _exact_rotations():
    m = lambda rows: np.array(rows, f32)
    table = [("perm_a", m([[0, 0, 1], [1, 0, 0], [0, 1, 0]]), 1, +1),      # trace exactly 0: not > 0, all diagonal entries equal: i = 0
             ("perm_b", m([[0, 1, 0], [0, 0, 1], [1, 0, 0]]), 1, -1),      # the raw w is -0.5: flipped
             ("half_x", m(np.diag([1, -1, -1])), 1, 0),                    # w = +0
             ("half_y", m(np.diag([-1, 1, -1])), 2, 0),
             ("half_z", m(np.diag([-1, -1, 1])), 3, 0),
             ("tie_01", m([[0, 1, 0], [1, 0, 0], [0, 0, -1]]), 1, 0),      # m00 == m11 the largest: the strict > keeps i = 0
             ("tie_12", m([[-1, 0, 0], [0, 0, 1], [0, 1, 0]]), 2, 0),      # m11 == m22 the largest: i = 1
             ("tie_02", m([[0, 0, 1], [0, -1, 0], [1, 0, 0]]), 1, 0)]      # m00 == m22 the largest: i = 0
    rng = np.random.Generator(np.random.PCG64(20260))
    for rep in range(4):                                                   # trace = 4 w^2 - 1 > 0: the first branch, both signs of w
        v = rng.uniform(-0.4, 0.4, 3)
        w = (0.7 + 0.25 * rng.uniform()) * (1 if rep % 2 == 0 else -1)
        table.append((f"rand_0_{rep}", _from_quat(v[0], v[1], v[2], w), 0, +1))
    for i in range(3):                                                     # |w| <= 0.3 of a dominant component near 1: trace < 0, branch 1 + i
        for rep in range(4):
            q = rng.uniform(-0.3, 0.3, 4)
            q[i] = (0.8 + 0.2 * rng.uniform()) * (1 if rep < 2 else -1)
            q[3] = (0.1 + 0.2 * rng.uniform()) * (1 if rep % 2 == 0 else -1)
            # Eigen's raw quaternion has q[i] > 0: its w has the sign of w * q[i]
            table.append((f"rand_{i + 1}_{rep}", _from_quat(q[0], q[1], q[2], q[3]), 1 + i, int(np.sign(q[3] * q[i]))))
    return table


EXACT_ROTATIONS = _exact_rotations()
N_EXACT_TABLE = 8                                                          # the first eight are exact in float32
TIES = ("tie_01", "tie_12", "tie_02")


def exact_problem(fixed_half=False):
    """one problem of len(EXACT_ROTATIONS) keyframes, no edges, three points nobody sees: no solver moves anything, and what comes back is
    the conversion of every float matrix to a quaternion and back"""
    K = len(EXACT_ROTATIONS)
    rng = np.random.Generator(np.random.PCG64(7))
    Tcw = np.zeros((K, 4, 4), f32)
    for k, (_, M, _, _) in enumerate(EXACT_ROTATIONS):
        Tcw[k, :3, :3] = M
        Tcw[k, :3, 3] = rng.normal(0, 2.0, 3)
        Tcw[k, 3, 3] = 1
    fixed = np.zeros(K, np.uint8)
    fixed[0] = 1
    if fixed_half:
        fixed[0::2] = 1
    z = np.zeros(0, f32)
    return dict(Tcw=Tcw, cam=np.tile(np.array([ls.FX, ls.FY, ls.CX, ls.CY, ls.BF], f32), (K, 1)), fixed=fixed,
                Xw=rng.normal(0, 1.0, (3, 3)).astype(f32), edge_kf=np.zeros(0, np.int32), edge_point=np.zeros(0, np.int32), x=z, y=z, u_right=z,
                inv_sigma2=z)
