"""Crowded, fully synthetic scenes for the BoW matchers: every feature is one of a few 32-byte prototypes with a small fraction of its
bits flipped, and its vocabulary node is drawn independently of the prototype (the recipe of tools/soak_bow.py, fixed and small).  A row
then has many columns within TH_LOW in its node, rows compete for columns, distances tie, and the ratio test is a real decision.  What
chance does not produce (a best distance of exactly 50, exact ratio equalities, a chain of displaced rows, rotations at bin boundaries) is
planted: a planted group sits on a fresh random descriptor, far from everything else, and its members differ from it in chosen bits.

Every scene is built once (functools.lru_cache) and its arrays are read-only."""
import functools

import numpy as np

from tools import synth

f32 = np.float32
SF = (f32(1.2) ** np.arange(8, dtype=f32)).astype(f32)       # mvScaleFactors / mvLevelSigma2 of the default extractor
SIG2 = (SF * SF).astype(f32)
RATIOS = (0.6, 0.75, 0.9)
TIE_RATIO = 1.25     # S-edges only: at a ratio <= 1 two columns tied at the smallest distance always fail the ratio test, so WHICH of them the
#                      walk holds cannot show; the reference takes any mfNNratio, and above 1 the first of them is matched


class Side:
    """feature lists of one side before they become a feature set"""

    def __init__(self):
        self.node, self.desc, self.flag, self.angle, self.x, self.y, self.octave, self.u_right = ([] for _ in range(8))

    def add(self, node, desc, flag=1, angle=0.0, x=0.0, y=0.0, octave=0, u_right=-1.0):
        self.node.append(int(node)); self.desc.append(np.asarray(desc, np.uint8)); self.flag.append(int(flag)); self.angle.append(f32(angle))
        self.x.append(f32(x)); self.y.append(f32(y)); self.octave.append(int(octave)); self.u_right.append(f32(u_right))
        return len(self.node) - 1

    def extend(self, node, desc, flag, angle, x=None, y=None, octave=None, u_right=None):
        n = len(node)
        z = np.zeros(n)
        for i in range(n):
            self.add(node[i], desc[i], flag[i], angle[i], (z if x is None else x)[i], (z if y is None else y)[i],
                     (z if octave is None else octave)[i], (z - 1 if u_right is None else u_right)[i])

    def featset(self):
        """FeatureVector as DBoW2 builds it: node ids ascending, the features of a node in ascending index order"""
        node = np.array(self.node, np.int64)
        order = np.argsort(node, kind="stable")
        ids, counts = np.unique(node, return_counts=True)
        off = np.zeros(len(ids) + 1, np.int32); off[1:] = np.cumsum(counts)
        fs = dict(desc=np.ascontiguousarray(np.stack(self.desc)), node_id=ids.astype(np.uint32), node_off=off, feat=order.astype(np.uint32),
                  flag=np.array(self.flag, np.uint8), angle=np.array(self.angle, f32), x=np.array(self.x, f32), y=np.array(self.y, f32),
                  octave=np.array(self.octave, np.int32), u_right=np.array(self.u_right, f32))
        for a in fs.values():
            a.setflags(write=False)
        return fs


def flipped(base, lo, hi):
    """`base` with bits lo .. hi-1 flipped: Hamming distance hi - lo from it"""
    bits = np.unpackbits(np.asarray(base, np.uint8))
    bits[lo:hi] ^= 1
    return np.packbits(bits)


def node_sizes(a, b):
    """(rows, columns) of every shared node"""
    ia = {int(i): int(a["node_off"][j + 1] - a["node_off"][j]) for j, i in enumerate(a["node_id"])}
    ib = {int(i): int(b["node_off"][j + 1] - b["node_off"][j]) for j, i in enumerate(b["node_id"])}
    return {i: (ia[i], ib[i]) for i in sorted(set(ia) & set(ib))}


def _crowd(rng, side, n, nodes, base, flip, proto_angle, rot, flag_p=0.8):
    """n features: a random prototype each, `flip` of its bits flipped; node from `nodes` (an array of n ids, or a count to draw from);
    angle = the prototype's + rot + N(0, 6), so that the rotation histogram has a peak with shoulders"""
    pid = rng.integers(0, len(base), n)
    node = nodes if isinstance(nodes, np.ndarray) else 10 + rng.integers(0, nodes, n)
    desc = synth.flip_bits(rng, base[pid], flip)
    flag = (rng.random(n) < flag_p).astype(np.uint8)
    angle = ((proto_angle[pid] + rot + rng.normal(0, 6, n)) % 360).astype(f32)
    side.extend(node, desc, flag, angle)


def _small_nodes(rng, a, b, base, first_node):
    """nodes of 1, 2, 3 and 3 columns against 5 rows each, near-duplicates of one prototype, all flagged: the rows of k_bow2's `complete`
    shortcut, the later ones with every column already taken"""
    for k, ncol in enumerate((1, 2, 3, 3)):
        for _ in range(5):
            a.add(first_node + k, synth.flip_bits(rng, base[:1], 0.02)[0], 1, rng.uniform(0, 360))
        for _ in range(ncol):
            b.add(first_node + k, synth.flip_bits(rng, base[:1], 0.02)[0], 1, rng.uniform(0, 360))


def _one_free_groups(rng, a, b, nodes, count=6):
    """`count` groups of 3 rows x 4 columns on a thermometer code of a fresh descriptor (positions: columns 0, 20, 24, 60; rows 20, 25, 2):
    the first two rows take the columns at 20 and 24, the third then has ONE free key among its three smallest -- (2, free), (18, taken),
    (22, taken) -- and 2 < ratio * 22 holds for every ratio used: k_bow2 decides it from that key and d3, without the walk"""
    for g in range(count):
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        for p in (20, 25, 2):
            a.add(nodes[g % len(nodes)], flipped(d, 0, p), 1, rng.uniform(0, 360))
        for p in (0, 20, 24, 60):
            b.add(nodes[g % len(nodes)], flipped(d, 0, p), 1, rng.uniform(0, 360))


def _tile_sides(plant=None):
    rng = np.random.Generator(np.random.PCG64(7))
    base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    pa = rng.uniform(0, 360, 4)
    sides = [Side() for _ in range(4)]
    for s, n, rot in zip(sides, (200, 200, 150, 260), (0.0, 40.0, 75.0, 200.0)):
        _crowd(rng, s, n, 8, base, 0.04, pa, rot)
    for s in sides[1:]:
        _small_nodes(rng, sides[0] if s is sides[1] else Side(), s, base, 100)
    _one_free_groups(rng, sides[0], sides[1], list(range(10, 18)))
    if plant:
        plant(rng, sides[0], sides[1])
    return [s.featset() for s in sides]


@functools.lru_cache(maxsize=None)
def s_tile():
    """200 + 200 features (+ the small nodes and the one-free-key groups) in 8 nodes of at most 64 x 64, 4 prototypes, flip 0.04
    -> (A, B, [B, B2, B3]): B2 / B3 are 150 and 260 features of the same prototypes, the neighbours of the batched calls"""
    a, b, b2, b3 = _tile_sides()
    assert all(r <= 64 and c <= 64 for r, c in node_sizes(a, b).values())
    return a, b, [b, b2, b3]


@functools.lru_cache(maxsize=None)
def s_large():
    """300 + 300 in 3 nodes, 6 prototypes, flip 0.06: node 10 over 64 on both sides, node 11 over 64 on the column side only, node 12 over 64
    on both; plus the small nodes and the one-free-key groups"""
    rng = np.random.Generator(np.random.PCG64(8))
    base = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    pa = rng.uniform(0, 360, 6)
    a, b = Side(), Side()
    _crowd(rng, a, 300, rng.permutation(np.repeat([10, 11, 12], (120, 60, 120))), base, 0.06, pa, 0.0)
    _crowd(rng, b, 300, rng.permutation(np.repeat([10, 11, 12], (110, 100, 90))), base, 0.06, pa, 40.0)
    _small_nodes(rng, a, b, base, 100)
    _one_free_groups(rng, a, b, [10, 12])
    a, b = a.featset(), b.featset()
    sz = node_sizes(a, b)
    assert sz[10] == (129, 122) and sz[11] == (60, 100) and sz[12] == (129, 102)
    return a, b


EDGE_ROWS = {}       # name -> first-side feature index (or indices) of a planted group of S-edges, filled by s_edges()


def _plant_edges(rng, a, b):
    nodes = [10 + k for k in range(8)]
    turn = [0]

    def group(name, cols, angle1=320.0, angle2=0.0):
        """one row on a fresh descriptor and columns at the given (lo, hi) flips of it, in this order, in the next node (by default at
        a rotation of 320, inside the peak of the crowd)"""
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        node = nodes[turn[0] % 8]; turn[0] += 1
        r = a.add(node, d, 1, angle1)
        for lo, hi in cols:
            b.add(node, flipped(d, lo, hi), 1, angle2)
        EDGE_ROWS.setdefault(name, []).append(r)
    group("d50", [(0, 50)])
    group("d49", [(0, 49)])
    group("d51", [(0, 51)])
    group("3_5", [(0, 3), (0, 5)])                  # float(0.6f) * 5.0f rounds to exactly 3.0f: rejected in float, accepted in double
    group("3_4", [(0, 3), (0, 4)])                  # 0.75f * 4 = 3 exactly: rejected either way, 3 < 3 is false
    group("9_12", [(0, 9), (0, 12)])
    group("tie_ab", [(0, 7), (7, 14)])              # two columns at distance 7, in both orders of the two descriptors
    group("tie_ba", [(7, 14), (0, 7)])
    # a chain: row i sits 4 bits from column i - 1 and 8 from column i on a thermometer code, so that each row, finding its nearest column
    # held by the row before it, takes the next one and displaces the row after it: one fixpoint round per link
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    for p in (1, 4, 16, 28, 40):
        EDGE_ROWS.setdefault("chain", []).append(a.add(nodes[3], flipped(d, 0, p), 1, 320.0))
    for p in (0, 12, 24, 36, 48):
        b.add(nodes[3], flipped(d, 0, p), 1, 0.0)
    # one-to-one pairs at distance 4 whose angles put chosen rotations into the histogram (bins by matcher_model.rotation_bin):
    # 15 -> x.5 exactly (bin 1; half-to-even would say 0), 45 and 345 (1.5 and 11.5 after the float product), 75 (2.5: bin 3, half-to-even
    # 2), 354.9 / 355.1 (bin 12 with the reference's factor 1/30), -0.0 (not negative: no 360 added, bin 0), -360 + one ulp (bin 0), and 890:
    # the only way to bin 30, which wraps to 0
    below360 = np.nextafter(f32(360), f32(0))
    for name, a1, a2, count in (("rot15", 115.0, 100.0, 4), ("rot45", 145.0, 100.0, 2), ("rot345", 5.0, 20.0, 2), ("rot75", 175.0, 100.0, 2),
                                ("rot354.9", 354.9, 0.0, 1), ("rot355.1", 355.1, 0.0, 1), ("rot-0", -0.0, 0.0, 1), ("rot-360", 0.0, below360, 1),
                                ("rot890", 890.0, 0.0, 6)):
        for _ in range(count):
            group(name, [(0, 4)], a1, a2)


@functools.lru_cache(maxsize=None)
def s_edges():
    """S-tile with the planted groups of _plant_edges appended (the last rows and columns of their nodes); EDGE_ROWS names their rows"""
    EDGE_ROWS.clear()
    a, b = _tile_sides(_plant_edges)[:2]
    assert all(r <= 64 and c <= 64 for r, c in node_sizes(a, b).values())
    return a, b


@functools.lru_cache(maxsize=None)
def s_passes():
    """k_bow2's passes -> dict of (A, B):
      rows   1100 first-side rows in 4 nodes of 275 against 60 columns each: the listed rows of one 256-node chunk exceed 1024 -> two passes
      fall   one node of 1100 rows (more than a pass holds: the fall_list path through node_greedy_wave) and an ordinary node after it
      chunks 300 shared nodes of 4 rows x 5 columns: a second 256-node chunk"""
    out = {}
    for name, seed, na, nb, nodes_a, nodes_b in (
            ("rows", 21, 1100, 240, np.repeat(np.arange(10, 14), 275), np.repeat(np.arange(10, 14), 60)),
            ("fall", 22, 1140, 100, np.repeat([10, 11], (1100, 40)), np.repeat([10, 11], (60, 40))),
            ("chunks", 23, 1200, 1500, np.repeat(np.arange(10, 310), 4), np.repeat(np.arange(10, 310), 5))):
        rng = np.random.Generator(np.random.PCG64(seed))
        base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        pa = rng.uniform(0, 360, 4)
        a, b = Side(), Side()
        _crowd(rng, a, na, rng.permutation(nodes_a), base, 0.04, pa, 0.0)
        _crowd(rng, b, nb, rng.permutation(nodes_b), base, 0.04, pa, 40.0)
        out[name] = (a.featset(), b.featset())
    return out


def _tri_side(rng, n, nodes, base, flip, centre, sigma_y, rot, pa, mp_p=0.25, stereo_p=0.3):
    """a side of S-tri: the prototype also fixes where the feature lies -- x = its centre's + N(0, 12), y = its centre's + N(0, sigma_y) --
    so that the columns within TH_LOW of a row (the same prototype) scatter about the row's epipolar line; flag = "already has a MapPoint\""""
    s = Side()
    pid = rng.integers(0, len(base), n)
    s.extend(nodes, synth.flip_bits(rng, base[pid], flip), (rng.random(n) < mp_p).astype(np.uint8),
             ((pa[pid] + rot + rng.normal(0, 6, n)) % 360).astype(f32), centre[pid, 0] + rng.normal(0, 12, n), centre[pid, 1] + rng.normal(0, sigma_y, n),
             rng.integers(0, 8, n), np.where(rng.random(n) < stereo_p, 5.0, -1.0))
    return s


@functools.lru_cache(maxsize=None)
def s_tri():
    """200 + 200 crowded features with positions, octaves and u_right (about 0.3 stereo) -> dict(A, B, B2, F12, epipole, F0); B2 is a third
    keyframe of 150 features for the batched calls.  The second camera
    is the first translated along x, so epipolar lines are rows (plus a small perturbation of F12, as tests/test_matchers_percall.py has it);
    the epipole lies on a prototype's centre, inside the cloud; node 10 holds 80 x 75 features (more than M_SPLIT_PAIRS = 4096 pairs: split
    by rows over several items); three planted rows match at distance exactly 50; F0 = the zero matrix (den == 0 for every row)"""
    rng = np.random.Generator(np.random.PCG64(9))
    base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    pa = rng.uniform(0, 360, 4)
    centre = np.stack([rng.uniform(200, 1000, 4), rng.uniform(80, 300, 4)], 1)
    a = _tri_side(rng, 200, rng.permutation(np.repeat([10, 11, 12, 13, 14], (80, 30, 30, 30, 30))), base, 0.04, centre, 3.0, 0.0, pa)
    b = _tri_side(rng, 200, rng.permutation(np.repeat([10, 11, 12, 13, 14], (75, 35, 30, 30, 30))), base, 0.04, centre, 3.0, 40.0, pa)
    b2 = _tri_side(rng, 150, rng.permutation(np.repeat([10, 11, 12, 13, 15], (30, 30, 30, 30, 30))), base, 0.04, centre, 3.0, 75.0, pa)
    for k in range(3):     # distance exactly 50, both stereo (no epipole test), the same position (on the line)
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        a.add(11 + k, d, 0, 10.0, 500.0 + k, 40.0, 0, 5.0)
        b.add(11 + k, flipped(d, 0, 50), 0, 330.0, 460.0 + k, 40.0, 0, 5.0)
    F12 = (np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32) + f32(2e-7) * rng.normal(0, 1, (3, 3)).astype(f32)).astype(f32)
    F12.setflags(write=False)
    return dict(A=a.featset(), B=b.featset(), B2=b2.featset(), F12=F12, epipole=(float(f32(centre[0, 0])), float(f32(centre[0, 1]))), F0=np.zeros((3, 3), f32))


# ------------------------------------------------------------------------------------------ the model's answers, computed once

def greedy_scenes():
    """name -> (A, B, ratios)"""
    out = {"tile": s_tile()[:2] + (RATIOS,), "large": s_large() + (RATIOS,), "edges": s_edges() + (RATIOS + (TIE_RATIO,),)}
    for k, (a, b) in s_passes().items():
        out["passes_" + k] = (a, b, (0.9,))
    return out


@functools.lru_cache(maxsize=None)
def model_greedy(scene, kind, ratio, ori):
    """(match, nmatches, report) of matcher_model.search_by_bow_<kind> on a scene of greedy_scenes()"""
    import matcher_model
    a, b, _ = greedy_scenes()[scene]
    return getattr(matcher_model, "search_by_bow_" + kind)(a, b, ratio, ori)


def tri_cases():
    """name -> (A, B, F12): the crowded pair, the same pair seen the other way round, the pair with F12 = 0, the smaller neighbour"""
    t = s_tri()
    return {"ab": (t["A"], t["B"], t["F12"]), "ba": (t["B"], t["A"], np.ascontiguousarray(t["F12"].T)), "f0": (t["A"], t["B"], t["F0"]),
            "ab2": (t["A"], t["B2"], t["F12"])}


@functools.lru_cache(maxsize=None)
def model_tri(case, ori, only_stereo):
    """(pairs, report) of matcher_model.search_for_triangulation on a case of tri_cases()"""
    import matcher_model
    a, b, F = tri_cases()[case]
    return matcher_model.search_for_triangulation(a, b, F, *s_tri()["epipole"], SF, SIG2, ori, only_stereo)


DB_CAP, DB_COUNTS, DB_NKF = 256, (220, 180), 9


@functools.lru_cache(maxsize=None)
def s_db_raw():
    """the crowded set for BowDatabase, whose frames get their FeatureVector from a vocabulary on the device: 2 frames and 9 keyframes of 4
    prototypes at flip 0.04, and a 4 x 4 vocabulary grown from the prototypes, read at level 1 (levelsup = 1: four nodes of about 50 features)
    -> dict(voc=(parent, leaf, desc, weight), desc [2, DB_CAP, 32], angle [2, DB_CAP], kf=[(desc, flag, angle)])"""
    rng = np.random.Generator(np.random.PCG64(10))
    base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    pa = rng.uniform(0, 360, 4)
    voc = synth.vocab_tree(11, 4, 2, stop_frac=0.0, data=base)
    desc = np.zeros((len(DB_COUNTS), DB_CAP, 32), np.uint8); angle = np.zeros((len(DB_COUNTS), DB_CAP), f32)
    for i, n in enumerate(DB_COUNTS):
        pid = rng.integers(0, 4, n)
        desc[i, :n] = synth.flip_bits(rng, base[pid], 0.04)
        angle[i, :n] = ((pa[pid] + rng.normal(0, 20, n)) % 360).astype(f32)      # wide: the rotations spread over five or six bins
    kf = []
    for k in range(DB_NKF):
        n = 150 + 12 * k
        pid = rng.integers(0, 4, n)
        kf.append((synth.flip_bits(rng, base[pid], 0.04), (rng.random(n) < 0.8).astype(np.uint8), ((pa[pid] + 40 + rng.normal(0, 20, n)) % 360).astype(f32)))
    return dict(voc=voc, desc=desc, angle=angle, kf=kf)


def s_db(oracle):
    """s_db_raw() as feature sets, the FeatureVectors by the oracle's vocabulary (the vocabulary is not what these tests are about)
    -> (frames, keyframes)"""
    raw = s_db_raw()
    ovoc = oracle.Vocabulary(4, 2, *raw["voc"])

    def fset(desc, flag, angle):
        t = ovoc.transform(desc, 1)
        return dict(desc=np.ascontiguousarray(desc), node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"], flag=flag, angle=angle)
    frames = [fset(raw["desc"][i, :n], np.zeros(n, np.uint8), raw["angle"][i, :n]) for i, n in enumerate(DB_COUNTS)]
    return frames, [fset(*k) for k in raw["kf"]]
