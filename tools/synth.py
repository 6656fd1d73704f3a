"""Seeded synthetic inputs for tests and bench: no datasets exist offline.

Images: low-frequency gradient + random-contrast rectangles / rotated rectangles / discs
+ N(0, 2^2) noise, uint8.  Stereo: right eye = left shifted by a per-row-band integer
disparity in [2, 80] px + independent noise.  BoW: a seeded two-level slice of a k=10
vocabulary tree (only tree level L-4=2 matters for DBoW2::FeatureVector with levelsup=4,
reference src/Frame.cc:464, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259).
"""
import numpy as np


def _texture(rng, h, w, nshapes):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = 96.0 + 48.0 * np.sin(xx / w * 2.1 + 0.3) * np.cos(yy / h * 1.7 + 0.9)
    for _ in range(nshapes):
        kind = rng.integers(0, 3)
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        sx, sy = rng.uniform(3, 0.03 * w + 6), rng.uniform(3, 0.06 * h + 6)
        val = rng.uniform(10, 245)
        x0, x1 = int(max(cx - 1.5 * sx - 2, 0)), int(min(cx + 1.5 * sx + 2, w))
        y0, y1 = int(max(cy - 1.5 * sy - 2, 0)), int(min(cy + 1.5 * sy + 2, h))
        if x1 <= x0 or y1 <= y0:
            continue
        sub_x, sub_y = xx[y0:y1, x0:x1] - cx, yy[y0:y1, x0:x1] - cy
        if kind == 0:
            m = (np.abs(sub_x) < sx) & (np.abs(sub_y) < sy)
        elif kind == 1:
            t = rng.uniform(0, np.pi)
            c, s = np.cos(t), np.sin(t)
            m = (np.abs(c * sub_x + s * sub_y) < sx) & (np.abs(-s * sub_x + c * sub_y) < sy)
        else:
            r = min(sx, sy)
            m = sub_x * sub_x + sub_y * sub_y < r * r
        blk = img[y0:y1, x0:x1]
        a = rng.uniform(0.5, 1.0)
        blk[m] = (1 - a) * blk[m] + a * val
    return img


def _finish(rng, img, sigma=2.0):
    out = img + rng.normal(0, sigma, img.shape).astype(np.float32)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def image(seed, w, h, nshapes=1500):
    rng = np.random.Generator(np.random.PCG64(seed))
    return _finish(rng, _texture(rng, h, w, nshapes))


def sequence(seed, w, h, nframes, nshapes=1500):
    """frames translating 1-3 px/frame over one wide texture"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pad = 3 * nframes + 4
    tex = _texture(rng, h + pad, w + pad, nshapes)
    out, ox, oy = [], 0, 0
    for _ in range(nframes):
        out.append(_finish(rng, tex[oy:oy + h, ox:ox + w]))
        ox += int(rng.integers(1, 4)); oy += int(rng.integers(0, 3))
    return np.stack(out)


def stereo_pair(seed, w, h, nshapes=1500, dmin=2, dmax=80):
    rng = np.random.Generator(np.random.PCG64(seed))
    tex = _texture(rng, h, w + dmax + 1, nshapes)
    nb = max(2, h // 47)
    edges = np.linspace(0, h, nb + 1).astype(int)
    disp = np.zeros(h, np.int64)
    for b in range(nb):
        disp[edges[b]:edges[b + 1]] = int(rng.integers(dmin, dmax + 1))
    # a scene point seen at column uL in the left eye is seen at uR = uL - d in the right eye
    # (positive disparity, src/Frame.cc:649):  right[y, u] = left[y, u + d]
    left = tex[:, :w]
    right = np.empty_like(left)
    for y in range(h):
        right[y] = tex[y, disp[y]:disp[y] + w]
    return _finish(rng, left), _finish(rng, right), disp


# ----------------------------------------------------------------------------- directed images for orientation / rBRIEF
# (tests/test_desc_model.py; 320 x 240, extracted with 8 levels at scale factor 1.2 and 500 features)

_DOT3 = np.array([[150, 200, 150], [200, 255, 200], [150, 200, 150]], np.uint8)   # brighter centre: a flat 3x3 plateau has no strict FAST maximum


def _dot_centres(w, h, pitch=40, x0=30, y0=30):
    return [(x, y) for y in range(y0, h - 25, pitch) for x in range(x0, w - 25, pitch)]


def _put_dot(img, x, y, big):
    if big:
        img[y - 1:y + 2, x - 1:x + 2] = _DOT3
    else:
        img[y, x] = 255


def isolated_dots(w=320, h=240, background=40):
    """1-pixel and 3x3 dots (alternating) on a constant background, 40 px apart: every patch of a level-0 keypoint is symmetric in
    both axes, so m10 = m01 = 0.  -> (image, [(x, y)])"""
    img = np.full((h, w), background, np.uint8)
    centres = _dot_centres(w, h)
    for i, (x, y) in enumerate(centres):
        _put_dot(img, x, y, i % 2 == 1)
    return img, centres


def dots_with_bar(w=320, h=240, background=40, bar=160):
    """the dots of isolated_dots, each with one 5 x 2 bar inside its 15-px patch, 7-8 px straight right of, below, left of or above the
    centre and symmetric about that axis: one moment is zero, the other has either sign (orientations 0, 90, 180, 270 degrees in
    image coordinates, y down).  -> (image, [(x, y, direction)]) with direction 0 = right, 1 = below, 2 = left, 3 = above"""
    img, centres = isolated_dots(w, h, background)
    out = []
    for i, (x, y) in enumerate(centres):
        d = (i + i // 7) % 4
        if d == 0:
            img[y - 2:y + 3, x + 7:x + 9] = bar
        elif d == 1:
            img[y + 7:y + 9, x - 2:x + 3] = bar
        elif d == 2:
            img[y - 2:y + 3, x - 8:x - 6] = bar
        else:
            img[y - 8:y - 6, x - 2:x + 3] = bar
        out.append((x, y, d))
    return img, out


def border_lattice(w=320, h=240, background=40, scale_factor=1.2, levels=4):
    """small squares (the 3x3 dot) along the four borders, phased so that for each of the first `levels` pyramid levels one of them
    is centred on the first (19) and one on the last (size - 20) admissible keypoint column and row of that level: a keypoint there
    has a rotated rBRIEF pattern that reaches row / column 1 of the level.  Level-l coordinate c is level-0 coordinate
    (c + 0.5) * scale - 0.5 (bilinear resize, pixel centres); the neighbouring phases +-1 px are placed too."""
    img = np.full((h, w), background, np.uint8)
    s = 1.0
    slot = 0
    for l in range(levels):
        lw, lh = int(round(w / s)), int(round(h / s))
        for ph in (-1, 0, 1):
            lo = int(round(19.5 * s - 0.5)) + ph
            hi_x = int(round((lw - 20 + 0.5) * s - 0.5)) + ph
            hi_y = int(round((lh - 20 + 0.5) * s - 0.5)) + ph
            ay, ax = 40 + 14 * slot, 50 + 19 * slot                # positions along the borders: 14 / 19 px between neighbours
            slot += 1
            for x, y in ((lo, ay), (min(hi_x, w - 3), ay + 7), (ax, lo), (ax + 9, min(hi_y, h - 3))):
                _put_dot(img, x, y, True)
        s *= scale_factor
    return img


def block_checkerboard(seed=7, w=320, h=240, block=16, flip=0.3):
    """0/255 checkerboard of 16-px blocks in which a seeded 30 % of the blocks are inverted: the crossing of four checkerboard blocks is
    no FAST-9 corner (two bright and two dark arcs of four pixels), the L-corners the inverted blocks make are.  After the 7x7 blur
    block interiors stay exactly 0 and 255 (both ends of the range), so many compared pixel pairs are equal."""
    rng = np.random.Generator(np.random.PCG64(seed))
    by, bx = (h + block - 1) // block, (w + block - 1) // block
    cells = (np.add.outer(np.arange(by), np.arange(bx)) & 1).astype(np.uint8)
    cells ^= (rng.random((by, bx)) < flip).astype(np.uint8)
    return (np.repeat(np.repeat(cells, block, 0), block, 1)[:h, :w] * 255).astype(np.uint8)


# ----------------------------------------------------------------------------- directed images for the cell grid of per-cell FAST
# (tests/test_front_model.py; 320 x 240 with 8 levels at scale factor 1.2 unless said otherwise)

def cell_lattice(size):
    """first detectable column (or row) of every FAST cell of a level `size` pixels wide (or high), src/ORBextractor.cc:934-976:
    cell j detects in [19 + j * cell, 19 + (j + 1) * cell) -> (starts, cell)"""
    extent = size - 32
    n = int(extent / 30)
    cell = -(-extent // n)
    return [19 + j * cell for j in range(n)], cell


def tie_bars(w=320, h=240, background=40):
    """pairs of adjacent single pixels of 255 on a flat background: both pixels of a pair have the same FAST score (214), so each
    suppresses the other and neither is kept, at either threshold.  Level-0 cells are 32 x 35 px from (19, 19).
      cell (row 1, column 1): the pair (60, 60) (61, 60) and the single pixel (70, 70) = background + 12 (score 11): empty at
        iniThFAST = 20 only after suppression, so the cell runs again at minThFAST = 7 and gives exactly the candidate (54, 54, 11);
      cell (1, 3): a horizontal pair alone: empty in both passes;
      cell (1, 5): a vertical and a diagonal pair.
    -> (image, dict of the pixel positions)"""
    img = np.full((h, w), background, np.uint8)
    pairs = dict(horizontal_with_weak=((60, 60), (61, 60)), horizontal=((125, 65), (126, 65)), vertical=((185, 60), (185, 61)),
                 diagonal=((200, 75), (201, 76)))
    for a, b in pairs.values():
        img[a[1], a[0]] = 255; img[b[1], b[0]] = 255
    weak = (70, 70)
    img[weak[1], weak[0]] = background + 12
    return img, dict(pairs=pairs, weak=weak)


def straddling_corners(w=320, h=240, background=40, weak=150, strong=255, scale_factor=1.2):
    """pairs of adjacent single pixels of unequal value (FAST scores weak - background - 1 and strong - background - 1).  Inside one
    cell the weaker pixel is suppressed.  Where a cell boundary runs between the two, each cell scores only its own pixel (the other
    lies outside its detectable area, where the score buffer is 0) and BOTH are kept.
      level 0 (y < 70): pairs across a vertical boundary (weaker left, weaker right), a horizontal one (weaker above, weaker below)
        and a cell corner (both diagonals), and the same three kinds inside a cell;
      level 1 (y >= 90): the same kinds at the level-0 position (c + 0.5) * scale_factor - 0.5 of level-1 boundaries c, each at
        the three phases -1, 0, +1 px (the resize spreads a pixel over two, so which phase puts the maximum just across the
        boundary is left to the phases).
    -> (image, dict: level-0 pixel positions 'across' [(weak, strong)] and 'inside' [(weak, strong)])"""
    img = np.full((h, w), background, np.uint8)

    def put(pw, ps):
        img[pw[1], pw[0]] = weak; img[ps[1], ps[0]] = strong
        return pw, ps
    xs0, _ = cell_lattice(w); ys0, _ = cell_lattice(h)
    bx = [x - 1 for x in xs0[1:]]; by = [y - 1 for y in ys0[1:]]          # last detectable column / row of cells 0, 1, ...
    across = [put((bx[1], 30), (bx[1] + 1, 30)), put((bx[2] + 1, 30), (bx[2], 30)),                     # vertical boundary
              put((30, by[0]), (30, by[0] + 1)), put((100, by[0] + 1), (100, by[0])),                   # horizontal boundary
              put((bx[0], by[0]), (bx[0] + 1, by[0] + 1)), put((bx[3] + 1, by[0]), (bx[3], by[0] + 1))]  # cell corner
    x_in = xs0[5]
    inside = [put((x_in + 6, 30), (x_in + 7, 30)), put((x_in + 21, 30), (x_in + 21, 31)), put((x_in + 11, 42), (x_in + 12, 43))]
    # level 1
    lw, lh = int(np.rint(np.float32(w) / np.float32(scale_factor))), int(np.rint(np.float32(h) / np.float32(scale_factor)))
    xs1, _ = cell_lattice(lw); ys1, _ = cell_lattice(lh)
    bx1 = [int(np.floor((x - 1 + 0.5) * scale_factor)) for x in xs1[1:]]  # level-0 position of the last column of level-1 cells 0, 1, ...
    by1 = [int(np.floor((y - 1 + 0.5) * scale_factor)) for y in ys1[1:]]
    for ph in (-1, 0, 1):
        put((bx1[1] + ph, 124 + 12 * ph), (bx1[1] + ph + 1, 124 + 12 * ph))
        put((165 + 10 * ph, by1[1] + ph), (165 + 10 * ph, by1[1] + ph + 1))
    corners = [(bx1[3], by1[2]), (bx1[4], by1[2]), (bx1[5], by1[2]), (bx1[3], by1[3]), (bx1[4], by1[3]), (bx1[5], by1[3]),
               (bx1[0], by1[2]), (bx1[0], by1[3]), (bx1[2], by1[3])]
    for (cx, cy), (px, py) in zip(corners, [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]):
        put((cx + px, cy + py), (cx + px + 1, cy + py + 1))
    return img, dict(across=across, inside=inside)


def one_cell_fallback(seed=31, w=320, h=240, cells=((1, 1), (1, 4), (1, 7), (4, 1), (4, 4), (4, 7))):
    """a textured scene in which the whole FAST window (detectable area + 3 px) of isolated level-0 cells (row, column) is replaced
    by its own low-contrast copy, contrast between minThFAST = 7 and iniThFAST = 20: such a cell finds nothing at 20 and runs again
    at 7, while its 8 neighbours, textured, do not.  -> (image, cells)"""
    img = image(seed, w, h)
    low = (100 + (img.astype(np.int32) - 100) // 8).astype(np.uint8)
    xs, cw = cell_lattice(w); ys, ch = cell_lattice(h)
    for i, j in cells:
        x0, y0 = xs[j] - 3, ys[i] - 3
        img[y0:y0 + ch + 6, x0:x0 + cw + 6] = low[y0:y0 + ch + 6, x0:x0 + cw + 6]
    return img, cells


# ----------------------------------------------------------------------------- BoW

_POPCNT = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming_matrix(a, b):
    """[na,32] x [nb,32] uint8 -> [na,nb] int"""
    x = a[:, None, :] ^ b[None, :, :]
    return _POPCNT[x].sum(axis=2).astype(np.int32)


class Vocab2:
    """Levels 1 and 2 of a seeded k=10 vocabulary tree; node ids in breadth-first order
    (root 0, level-1 nodes 1..10, level-2 nodes 11..110)."""

    def __init__(self, seed, k=10):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.k = k
        self.l1 = rng.integers(0, 256, (k, 32), dtype=np.uint8)
        self.l2 = rng.integers(0, 256, (k, k, 32), dtype=np.uint8)

    def seed_from(self, desc, rng):
        """re-seed node descriptors from data so that features spread over nodes"""
        k = self.k
        self.l1 = desc[rng.choice(len(desc), k, replace=False)].copy()
        self.l2 = desc[rng.choice(len(desc), k * k, replace=False)].reshape(k, k, 32).copy()

    def node_of(self, desc):
        c1 = hamming_matrix(desc, self.l1).argmin(axis=1)  # first minimum, strict <
        out = np.empty(len(desc), np.uint32)
        for c in range(self.k):
            m = np.nonzero(c1 == c)[0]
            if len(m):
                c2 = hamming_matrix(desc[m], self.l2[c]).argmin(axis=1)
                out[m] = 1 + self.k + c * self.k + c2
        return out

    def feature_vector(self, desc):
        """CSR FeatureVector: (node_id ascending u32, node_off i32, feat ascending-in-node u32)"""
        node = self.node_of(desc)
        order = np.argsort(node, kind="stable")
        ids, counts = np.unique(node, return_counts=True)
        off = np.zeros(len(ids) + 1, np.int32)
        off[1:] = np.cumsum(counts)
        return ids.astype(np.uint32), off, order.astype(np.uint32)


def flip_bits(rng, desc, p):
    bits = np.unpackbits(desc, axis=1)
    bits ^= (rng.random(bits.shape) < p).astype(np.uint8)
    return np.packbits(bits, axis=1)


def vocab_tree(seed, k=10, L=3, stop_frac=0.02, data=None):
    """Seeded FULL k-ary vocabulary tree with node ids assigned LEVEL BY LEVEL (breadth-first): returns
    parent[], is_leaf[], desc[], weight[] for nodes 1..N (the root is implicit).  This is a valid
    vocabulary file, but NOT the order DBoW2 gives its own trees: HKmeansStep numbers the children of
    one node, then recurses into the first of them (TemplatedVocabulary.h:786-818), and
    saveToTextFile / loadFromTextFile keep that order -- see vocab_tree_dbow2.  Leaf weights are
    positive idf-like values, a fraction is 0 ("stopped" words, TemplatedVocabulary.h:1157).  Node
    descriptors are random, or sampled from `data` descriptors (+ bit noise) so that real features
    spread over the tree."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, leaf = [], []
    level_nodes = [0]
    next_id = 1
    for lvl in range(1, L + 1):
        new = []
        for p in level_nodes:
            for _ in range(k):
                parent.append(p); leaf.append(1 if lvl == L else 0); new.append(next_id); next_id += 1
        level_nodes = new
    n = len(parent)
    if data is not None:
        desc = flip_bits(rng, data[rng.integers(0, len(data), n)], 0.1)
    else:
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = np.where(np.array(leaf) == 1, rng.uniform(0.5, 9.0, n), 0.0)
    weight[(np.array(leaf) == 1) & (rng.random(n) < stop_frac)] = 0.0
    return np.array(parent, np.int32), np.array(leaf, np.uint8), desc, weight


def _split_descriptors(rng, m, c, single_frac, minimum=None):
    """m training descriptors over c clusters, none of them empty (TemplatedVocabulary.h:753); a seeded share of the clusters
    keeps a single descriptor, the others share the rest unevenly"""
    cnt = np.ones(c, np.int64) if minimum is None else np.asarray(minimum, np.int64).copy()
    rest = m - int(cnt.sum())
    assert rest >= 0, "not enough descriptors for the forced sibling groups"
    if rest > 0:
        grows = (rng.random(c) >= single_frac) | (cnt > 1)
        if not grows.any():
            grows[int(rng.integers(0, c))] = True
        p = rng.gamma(1.0, 1.0, c) * grows
        cnt += rng.multinomial(rest, p / p.sum())
    return cnt


def vocab_tree_dbow2(seed, k=10, L=6, n_feat=12000, stop_frac=0.02, noise=0.1, dup_frac=0.1, dup910_frac=0.5, single_frac=0.2,
                     groups_l1=()):
    """Seeded RAGGED vocabulary tree numbered and shaped as DBoW2 builds one from `n_feat` training descriptors
    (TemplatedVocabulary::HKmeansStep, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:642-819), without running k-means: only how many
    descriptors each cluster holds is carried down.  Same four arrays as vocab_tree.

      * a node holding m <= k descriptors gets one child per descriptor (:660-670); one holding more gets between k/2 and k (seeded;
        k-means gives at most k, and fewer when initial centres coincide);
      * ALL children of a node get consecutive ids first (:786-793) ...
      * ... then each child holding more than one descriptor is expanded in turn while level < L (:796-817); a child with a single
        descriptor stays a leaf at whatever level it is (:813).  So ids are neither level by level nor is a node's breadth-first
        position its id, and leaves sit at every level.

    Child descriptors are the parent's with `noise` bit noise (level 1: random).  A `dup_frac` share of siblings are exact copies of
    the sibling before them, so distance ties between DIFFERENT subtrees are certain (first minimum wins, strict <, :1244); in a
    `dup910_frac` share of the groups of more than ten children, child 10 also copies child 9 (a tie across the device's ten-child
    trips).  `groups_l1[i]` forces the number of children of the i-th level-1 node (a test lever: sibling groups of 1, 10, 11 or 20
    where k allows; HKmeansStep itself makes a group of one only when all centres coincide).  Weights as in vocab_tree: idf-like
    on leaves, a `stop_frac` share 0."""
    rng = np.random.Generator(np.random.PCG64(seed))
    assert 2 <= k <= 20 and 1 <= L <= 10 and len(groups_l1) <= k and all(1 <= g <= k for g in groups_l1)
    parent, desc = [], []          # nodes 1..N in id order
    nchild = [0]                   # per node, the root included

    def step(parent_id, parent_desc, m, level, forced=None):        # HKmeansStep(parent_id, descriptors, current_level), m = descriptors.size()
        if forced is not None:
            c = forced
        elif m <= k:
            c = m                                                    # :660-670
        else:
            c = int(rng.integers(max(1, k // 2), k + 1))
        minimum = None
        if level == 1 and groups_l1:
            c = max(c, len(groups_l1))
            minimum = np.ones(c, np.int64)
            minimum[:len(groups_l1)] = [max(2 * g, 2) for g in groups_l1]
        cnt = _split_descriptors(rng, m, c, single_frac, minimum)
        if parent_desc is None:
            d = rng.integers(0, 256, (c, 32), dtype=np.uint8)
        else:
            d = flip_bits(rng, np.repeat(parent_desc[None, :], c, axis=0), noise)
        dup = rng.random(c) < dup_frac
        for i in range(1, c):
            if dup[i]:
                d[i] = d[i - 1]
        if c > 10 and rng.random() < dup910_frac:
            d[10] = d[9]
        first = len(parent) + 1
        for i in range(c):                                           # create nodes: all children first (:786-793)
            parent.append(parent_id); desc.append(d[i]); nchild.append(0)
        nchild[parent_id] = c
        if level < L:                                                # :796
            for i in range(c):
                if cnt[i] > 1:                                       # :813
                    step(first + i, d[i], int(cnt[i]), level + 1,
                         groups_l1[i] if level == 1 and i < len(groups_l1) else None)

    step(0, None, int(n_feat), 1)                                    # create(): HKmeansStep(0, features, 1)
    n = len(parent)
    leaf = (np.array(nchild[1:]) == 0).astype(np.uint8)              # isLeaf() == children.empty() (:328)
    weight = np.where(leaf == 1, rng.uniform(0.5, 9.0, n), 0.0)
    weight[(leaf == 1) & (rng.random(n) < stop_frac)] = 0.0
    return np.array(parent, np.int32), leaf, np.array(desc, np.uint8).reshape(n, 32), weight


def vocab_features(seed, is_leaf, desc, n, noise=0.04):
    """n features for a vocabulary: descriptors of seeded leaves with `noise` bit noise"""
    rng = np.random.Generator(np.random.PCG64(seed))
    leaves = np.nonzero(np.asarray(is_leaf) == 1)[0]
    return flip_bits(rng, desc[leaves[rng.integers(0, len(leaves), n)]], noise)


def write_vocab_text(path, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
    """the ORBvoc.txt text format read by TemplatedVocabulary::loadFromTextFile (:1358-1445)"""
    with open(path, "w") as f:
        f.write(f"{k} {L} {scoring} {weighting}\n")
        for i in range(len(parent)):
            f.write(f"{parent[i]} {is_leaf[i]} " + " ".join(str(int(b)) for b in desc[i]) + f" {float(weight[i])!r}\n")
