"""Plain-Python model of the DBoW2 vocabulary transform, written from the reference's text with dict / list standing in for
std::map / std::vector.  It pins the CPU oracle (and through it the HIP path) where nothing of the reference can be compiled:
TemplatedVocabulary.h and FORB.cpp need OpenCV.

Reference lines (Thirdparty/DBoW2/DBoW2/):
  * TemplatedVocabulary.h:1127-1194  transform(features, BowVector, FeatureVector, levelsup): per feature, in feature order, the word's
    weight is added to the BowVector and the feature index appended under its node unless the word is stopped (:1157), then normalize;
  * TemplatedVocabulary.h:1218-1259  transform(feature, word_id, weight, nid, levelsup): the descent -- the children of the current node in
    the order of its children vector, first minimum wins (strict <, :1244), the node of level L - levelsup is remembered (:1251), the
    descent ends on the first node without children (:1254);
  * TemplatedVocabulary.h:1425-1432  loadFromTextFile: node ids are line numbers, children are pushed in id order (:1409), word ids are
    handed to the leaves in id order;
  * BowVector.cpp:33-77  addWeight (insert, or += in call order) and normalize(L1) (sum of |v| in ascending word order, then v / norm).

Defined deviation from the reference, the same one the oracle and the device make:
  * the node id of a feature is 0 when its descent ends on a leaf ABOVE level L - levelsup > 0.  The reference then never writes *nid
    (:1251 is not reached with current_level == nid_level) and the caller's `NodeId nid` (:1151) is uninitialised: whatever the stack
    held goes into the FeatureVector.  0, the root, is what :1227 gives a feature when the level is not positive.

tree_stats / descent_stats measure how far a vocabulary and a feature set are from the level-by-level full trees on which a breadth-first
renumbering is the identity; tests assert floors on them so that a tamer generator cannot quietly empty the tests."""
import numpy as np

POP = np.array([bin(i).count("1") for i in range(256)])


def children_lists(parent):
    """children[i] of node i (0 = root) in id order, as loadFromTextFile pushes them (:1409)"""
    children = [[] for _ in range(len(parent) + 1)]
    for i, p in enumerate(parent):
        children[p].append(i + 1)
    return children


def descend(children, ndesc, f):
    """:1229-1254 for one feature -> [(children of the node left, their distances, the child taken)] per level, level 1 first"""
    path, node = [], 0
    while True:
        ch = children[node]
        ds = [int(POP[f ^ ndesc[c - 1]].sum()) for c in ch]
        node = ch[int(np.argmin(ds))]          # first minimum
        path.append((ch, ds, node))
        if not children[node]:
            return path


def python_transform(k, L, parent, is_leaf, ndesc, weight, feats, levelsup):
    """-> (BowVector ids, BowVector values, {node id: [features]}) in ascending id order"""
    n = len(parent) + 1
    children = children_lists(parent)
    word = {}
    for i in range(1, n):
        if is_leaf[i - 1]:
            word[i] = len(word)
    bow, fv = {}, {}
    for fi, f in enumerate(feats):
        nid = 0                                    # stays 0 on a leaf above L - levelsup (defined deviation) and for L - levelsup <= 0 (:1227)
        for level, (_, _, node) in enumerate(descend(children, ndesc, f), 1):
            if level == L - levelsup:
                nid = node
        w = weight[node - 1]
        if w > 0:
            bow[word[node]] = bow.get(word[node], 0.0) + w if word[node] in bow else w
            fv.setdefault(nid, []).append(fi)
    ids = sorted(bow)
    vals = [bow[i] for i in ids]
    norm = 0.0
    for v in vals:
        norm += abs(v)
    if norm > 0:
        vals = [v / norm for v in vals]
    return ids, vals, {k_: fv[k_] for k_ in sorted(fv)}


def python_descent(L, parent, is_leaf, ndesc, weight, feats, levelsup):
    """per feature (word id, word weight, node id), as the oracle and the device return them next to the two vectors, and the level of
    the leaf the descent ended on"""
    children = children_lists(parent)
    word, nw = {}, 0
    for i in range(1, len(parent) + 1):
        if is_leaf[i - 1]:
            word[i] = nw; nw += 1
    wid, ww, nid, depth = [], [], [], []
    for f in feats:
        path = descend(children, ndesc, f)
        node = path[-1][2]
        wid.append(word[node]); ww.append(float(weight[node - 1]))
        nid.append(path[L - levelsup - 1][2] if 0 < L - levelsup <= len(path) else 0)
        depth.append(len(path))
    return wid, ww, nid, depth


def tree_stats(parent):
    """-> dict: bfs_pos[i] = position of node i (root included, position 0) when the tree is walked breadth-first with children in id
    order -- the order the device keeps the nodes in --, level[i], group_sizes = the set of sibling-group sizes present, moved = how many
    nodes sit at a position different from their id, nodes = node count (root included)"""
    children = children_lists(parent)
    n = len(children)
    order, level = [0], np.zeros(n, np.int64)
    for x in order:                                # grows while it is walked
        for c in children[x]:
            level[c] = level[x] + 1
            order.append(c)
    assert len(order) == n
    bfs_pos = np.empty(n, np.int64)
    bfs_pos[np.array(order)] = np.arange(n)
    return dict(bfs_pos=bfs_pos, level=level, group_sizes={len(c) for c in children if c},
                moved=int((bfs_pos != np.arange(n)).sum()), nodes=n)


def descent_stats(L, parent, ndesc, feats):
    """how many of `feats` -> dict: end_moved = end on a node whose breadth-first position differs from its id, leaf_above_L = end on a
    leaf above level L, tied = pass a level whose minimum distance is shared by two or more children, tied_across_ten = have such a
    tie with its first member among children 0..9 of the group and another member at position 10 or later, past_ten = take, at some
    level, a child at position 10 or later of its group (what a descent that looks at the first ten children only gets wrong)"""
    children = children_lists(parent)
    pos = tree_stats(parent)["bfs_pos"]
    out = dict(end_moved=0, leaf_above_L=0, tied=0, tied_across_ten=0, past_ten=0, n=len(feats))
    for f in feats:
        path = descend(children, ndesc, f)
        node = path[-1][2]
        out["end_moved"] += int(pos[node] != node)
        out["leaf_above_L"] += int(len(path) < L)
        tied = across = past = False
        for _, ds, _ in path:
            at = [j for j, d in enumerate(ds) if d == min(ds)]
            tied |= len(at) > 1
            across |= len(at) > 1 and at[0] < 10 and at[-1] >= 10
            past |= at[0] >= 10
        out["tied"] += int(tied); out["tied_across_ten"] += int(across); out["past_ten"] += int(past)
    return out
