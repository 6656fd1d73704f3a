"""Frame::ComputeBoW on vocabularies numbered and shaped as DBoW2 builds them (tools/synth.vocab_tree_dbow2: ids in HKmeansStep order,
ragged sibling groups, leaves at every level, k up to 20).  On the level-by-level full trees of synth.vocab_tree the breadth-first
renumbering of vocab_build (orbx_vocab.hip) is the identity and k_vocab_descend never takes a second ten-child trip, so neither is seen
by tests/test_vocab.py.  CPU: the oracle against the plain-Python model of tests/vocab_model.py, with floors on how un-tame the trees
and feature sets are.  GPU: the HIP path against the oracle, byte-equal."""
import functools
import os

import numpy as np
import pytest

import vocab_model as vm
from tools import synth

# name -> (vocab_tree_dbow2 arguments, levelsup).  Seeds: a tree of L = 3 keeps the breadth-first position of every deepest node below
# its LAST level-1 node (both orders end with them), so the seeds of those cases are ones whose last level-1 cluster came out small;
# the floors of test_oracle_vs_model_dbow2_order hold them there.
CASES = {
    "k10_L6_up4": (dict(seed=100, k=10, L=6, n_feat=24000), 4),                     # the call ORB-SLAM2 makes (src/Frame.cc:464), ~17 k nodes
    "k20_L3_up1": (dict(seed=109, k=20, L=3, n_feat=2000, single_frac=0.5, groups_l1=(1, 10, 11, 20)), 1),
    "k12_L4_up2": (dict(seed=100, k=12, L=4, n_feat=3000), 2),
    "k3_L10_up7": (dict(seed=110, k=3, L=10, n_feat=3000), 7),
    "k10_L3_up0": (dict(seed=151, k=10, L=3, n_feat=600, single_frac=0.3), 0),
    # GPU only: two ten-child trips, the second part-filled
    "k11_L4_up2": (dict(seed=134, k=11, L=4, n_feat=4000), 2),
    "k16_L3_up1": (dict(seed=104, k=16, L=3, n_feat=2000), 1),
    # GPU only: the tree of the k_bow_build sort-path test
    "k10_L4_up2": (dict(seed=102, k=10, L=4, n_feat=2500), 2),
}
FIVE = ["k10_L6_up4", "k20_L3_up1", "k12_L4_up2", "k3_L10_up7", "k10_L3_up0"]
NFEAT = 1000


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (k, L, levelsup, (parent, is_leaf, desc, weight), 1000 features: leaf descriptors with 4 % bit noise); built once, never written to"""
    args, levelsup = CASES[name]
    tree = synth.vocab_tree_dbow2(**args)
    feats = synth.vocab_features(args["seed"] + 1000, tree[1], tree[2], NFEAT, 0.04)
    for a in tree + (feats,):
        a.setflags(write=False)
    return args["k"], args["L"], levelsup, tree, feats


_EXPECT = {}


def _expect(oracle, name):
    """the oracle's transform of the case's features (shared, read-only)"""
    if name not in _EXPECT:
        k, L, levelsup, tree, feats = _case(name)
        _EXPECT[name] = oracle.Vocabulary(k, L, *tree).transform(feats, levelsup)
    return _EXPECT[name]


def _cmp(a, b, what=""):
    for k_ in a:
        assert a[k_].dtype == b[k_].dtype and a[k_].shape == b[k_].shape, (what, k_)
        assert a[k_].tobytes() == b[k_].tobytes(), (what, k_)


def test_generator_numbers_nodes_as_hkmeansstep():
    """the ids of vocab_tree_dbow2 are those of HKmeansStep (TemplatedVocabulary.h:786-818): the children of a node are consecutive, and the
    groups follow each other in the order of a walk that expands a node's children first to last, each before its next sibling"""
    for name in ("k20_L3_up1", "k3_L10_up7", "k12_L4_up2"):
        k, L, _, (par, leaf, nd, w), _ = _case(name)
        children = vm.children_lists(par)
        assert all(ch == list(range(ch[0], ch[0] + len(ch))) for ch in children if ch)
        assert all(1 <= len(ch) <= k for ch in children if ch)
        nxt, stack = 1, [0]
        while stack:
            x = stack.pop()
            assert children[x][0] == nxt                 # the group of the node expanded next starts right after everything numbered so far
            nxt += len(children[x])
            stack.extend(c for c in reversed(children[x]) if children[c])
        assert nxt == len(par) + 1
        st = vm.tree_stats(par)
        assert st["level"].max() == L
        assert (leaf == np.array([0 if children[i] else 1 for i in range(1, len(par) + 1)], np.uint8)).all()   # isLeaf() == children.empty()
        assert ((w > 0) <= (leaf == 1)).all() and nd.shape == (len(par), 32)
        again = synth.vocab_tree_dbow2(**CASES[name][0])
        assert all((a == b).all() for a, b in zip(again, (par, leaf, nd, w)))


@pytest.mark.parametrize("name", FIVE)
def test_oracle_vs_model_dbow2_order(oracle, name):
    k, L, levelsup, (par, leaf, nd, w), feats = _case(name)
    t = _expect(oracle, name)
    # ---- validity: the tree and the features are what the old generator could not give
    ts = vm.tree_stats(par); ds = vm.descent_stats(L, par, nd, feats)
    print(name, "nodes", ts["nodes"], "moved", ts["moved"], "group sizes", sorted(ts["group_sizes"]), ds)
    assert ts["moved"] >= 0.75 * ts["nodes"]             # nodes whose breadth-first position differs from their id
    assert ds["end_moved"] >= 0.90 * NFEAT               # features that end on such a node
    assert ds["leaf_above_L"] >= 100                     # features that end on a leaf above level L
    assert ds["tied"] >= 100                             # features that pass a level with a shared minimum
    if k > 10:
        assert ds["tied_across_ten"] >= 20               # ... shared between children 0..9 and children 10.. of one group
        assert ds["past_ten"] >= 20                      # features that take a child at position 10 or later (the floor of the tie above)
    if k == 3:
        assert 1 in ts["group_sizes"]
    if k == 20:
        assert {1, 10, 11, 20} <= ts["group_sizes"]
    # ---- oracle == model
    ov = oracle.Vocabulary(k, L, par, leaf, nd, w)
    assert ov.nodes() == len(par) + 1 and ov.words() == int(leaf.sum())
    ids, vals, fv = vm.python_transform(k, L, par, leaf, nd, w, feats, levelsup)
    assert t["bow_id"].tolist() == ids
    assert t["bow_val"].tolist() == vals                 # identical doubles
    assert t["fv_node_id"].tolist() == list(fv)
    for j, nid in enumerate(fv):
        assert t["fv_feat"][t["fv_node_off"][j]:t["fv_node_off"][j + 1]].tolist() == fv[nid]
    wid, ww, nid, depth = vm.python_descent(L, par, leaf, nd, w, feats, levelsup)
    assert t["word_id"].tolist() == wid and t["word_weight"].tolist() == ww and t["node_id"].tolist() == nid
    short = np.array(depth) < L - levelsup               # leaf above L - levelsup: node id 0 (defined deviation, vocab_model.py)
    print(name, "features ending above level L - levelsup:", int(short.sum()))
    assert (t["node_id"][short] == 0).all() and (t["node_id"][~short] != 0).all() == (L - levelsup > 0)
    if name in ("k3_L10_up7", "k10_L3_up0"):             # the cases that carry this edge (the others need not: few leaves sit that high)
        assert short.sum() >= 20


@pytest.mark.parametrize("name", FIVE)
def test_oracle_text_roundtrip_dbow2_order(oracle, tmp_path, name):
    k, L, levelsup, (par, leaf, nd, w), feats = _case(name)
    path = os.path.join(tmp_path, "voc.txt")
    synth.write_vocab_text(path, k, L, par, leaf, nd, w)
    ov = oracle.Vocabulary(path=path)
    assert ov.nodes() == len(par) + 1 and ov.words() == int(leaf.sum())
    _cmp(ov.transform(feats, levelsup), _expect(oracle, name), name)


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("name", FIVE + ["k11_L4_up2", "k16_L3_up1"])
def test_hip_transform_parity_dbow2_order(pkg, oracle, name):
    k, L, levelsup, tree, feats = _case(name)
    got = pkg.ORBVocabulary(k, L, *tree).transform(feats, levelsup)
    exp = _expect(oracle, name)
    if k > 10:                                           # (the k = 11 and k = 16 trees have no CPU test of their own)
        ds = vm.descent_stats(L, tree[0], tree[2], feats)
        assert ds["tied_across_ten"] >= 20 and ds["past_ten"] >= 20, ds
    for key in ("word_id", "word_weight", "node_id"):    # the descent first, so that a failure names it and not the build of the two vectors
        bad = np.nonzero(got[key] != exp[key])[0]
        assert len(bad) == 0, (name, key, len(bad), bad[:5].tolist(), got[key][bad[:5]].tolist(), exp[key][bad[:5]].tolist())
    _cmp(got, exp, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k10_L6_up4", "k20_L3_up1"])
def test_hip_loader_dbow2_order(pkg, oracle, tmp_path, name):
    k, L, levelsup, (par, leaf, nd, w), feats = _case(name)
    path = os.path.join(tmp_path, "voc.txt")
    synth.write_vocab_text(path, k, L, par, leaf, nd, w)
    voc = pkg.ORBVocabulary.loadFromTextFile(path)
    assert voc.info() == dict(k=k, L=L, nodes=len(par) + 1, words=int(leaf.sum()))
    got = voc.transform(feats, levelsup)
    _cmp(got, pkg.ORBVocabulary(k, L, par, leaf, nd, w).transform(feats, levelsup), name)
    _cmp(got, _expect(oracle, name), name)


@pytest.mark.gpu
def test_hip_bow_build_sort_paths_ragged_tree(pkg, oracle):
    """every sort form of k_bow_build at its power of two and one past it (npad 64 .. 8192: the LDS network, the two register forms at
    1024 and 2048, the limit of two key sets in LDS at 4096, one key set above), on node ids that do not grow with the device's order"""
    k, L, levelsup, tree, _ = _case("k10_L4_up2")
    feats = synth.vocab_features(7, tree[1], tree[2], 8193, 0.04)
    voc = pkg.ORBVocabulary(k, L, *tree); ovoc = oracle.Vocabulary(k, L, *tree)
    for n in (1, 64, 65, 128, 129, 256, 1024, 1025, 2048, 2049, 4096, 4097, 8192):
        _cmp(voc.transform(feats[:n], levelsup), ovoc.transform(feats[:n], levelsup), n)
    with pytest.raises(pkg.OrbxError):
        voc.transform(feats, levelsup)                   # 8193 features
    # one word, its weight added 1024 times in feature order
    live = np.nonzero(ovoc.transform(feats[:64], levelsup)["word_weight"] > 0)[0]
    same = np.repeat(feats[live[0]:live[0] + 1], 1024, axis=0)
    exp = ovoc.transform(same, levelsup)
    assert len(exp["bow_id"]) == 1 and len(exp["fv_feat"]) == 1024
    _cmp(voc.transform(same, levelsup), exp, "identical")


def _batch_scene(oracle, name, cap):
    """CPU side of the batched test: 4 frames of `cap` keypoints and descriptors (numpy, no extraction), counts 0, 1, cap and cap + 77,
    the oracle's transform per frame (of the first min(count, cap) features), 4 keyframes made from frames 2 and 3, and the oracle's
    SearchByBoW result per (frame, keyframe)"""
    k, L, levelsup, tree, _ = _case(name)
    B = 4
    rng = np.random.Generator(np.random.PCG64(cap))
    desc = synth.vocab_features(cap + 1, tree[1], tree[2], B * cap, 0.04).reshape(B, cap, 32)
    kps = np.zeros((B, cap, 7), np.float32)              # cv::KeyPoint records: x, y, size, angle, response, octave, class_id
    kps[:, :, 3] = rng.uniform(0, 360, (B, cap)).astype(np.float32)
    counts = np.array([0, 1, cap, cap + 77], np.int32)
    n = np.minimum(counts, cap)
    ovoc = oracle.Vocabulary(k, L, *tree)
    frames, exp_t = [], []
    for i in range(B):
        t = ovoc.transform(desc[i, :n[i]], levelsup)
        exp_t.append(t)
        frames.append(dict(desc=desc[i, :n[i]], node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"],
                           flag=np.zeros(n[i], np.uint8), angle=kps[i, :n[i], 3].copy()))
    kfs = []
    for j in range(4):
        base = frames[2 + j % 2]
        perm = rng.permutation(cap); dk = synth.flip_bits(rng, base["desc"], 0.05)[perm]
        t = ovoc.transform(dk, levelsup)
        kfs.append(dict(desc=dk, node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"],
                        flag=(rng.random(cap) < 0.7).astype(np.uint8), angle=base["angle"][perm]))
    expect = [[oracle.search_by_bow_kf_f(kf, frames[i], 0.75, True) for kf in kfs] for i in range(B)]
    return dict(desc=desc, kps=kps, counts=counts, n=n, exp_t=exp_t, kfs=kfs, expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1000, 300])
@pytest.mark.parametrize("name", ["k10_L6_up4", "k20_L3_up1"])
def test_hip_batched_bow_and_search_dbow2_order(pkg, oracle, name, cap):
    """orbx_bow_transform_batch_device on uploaded descriptors (counts 0, 1, cap and one above cap, which must clamp), then every frame
    against a 4-keyframe BowDatabase in both forms of the search kernel.  The FeatureVectors' node ids are DBoW2 ids, which do not grow
    with the device's node order: the merge of the two sorted node lists is what the search part checks.  The oracle gives
    2737 (k10_L6_up4) and 2749 (k20_L3_up1) matches over the 16 pairs at cap 1000, 825 and 838 at cap 300."""
    import torch
    k, L, levelsup, tree, _ = _case(name)
    B = 4
    sc = _batch_scene(oracle, name, cap)
    n, kfs, expect = sc["n"], sc["kfs"], sc["expect"]
    total_exp = sum(en for row in expect for _, en in row)
    print(name, cap, "oracle matches in all:", total_exp)
    assert total_exp > 0
    d_kps = torch.from_numpy(sc["kps"]).cuda(); d_desc = torch.from_numpy(sc["desc"].copy()).cuda(); d_n = torch.from_numpy(sc["counts"]).cuda()
    stream = torch.cuda.Stream(); st = stream.cuda_stream
    torch.cuda.synchronize()
    voc = pkg.ORBVocabulary(k, L, *tree)
    fr = pkg.BowFrames(B, cap)
    fr.transform(voc, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), B, levelsup, st)
    for i in range(B):
        got = fr.read(i, st); exp = sc["exp_t"][i]
        for k_ in ("bow_id", "fv_node_id", "fv_node_off", "fv_feat"):
            assert got[k_].shape == exp[k_].shape and (got[k_] == exp[k_]).all(), (i, k_)
        assert got["bow_val"].tobytes() == exp["bow_val"].tobytes(), i       # doubles, bit-exact
    db = pkg.BowDatabase(kfs)
    d_match = torch.full((B, len(kfs), cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.zeros((B, len(kfs)), dtype=torch.int32, device="cuda")
    for form in ("table", "wave"):
        pkg.orbx.debug_set_bow_form(form)
        try:
            d_match.fill_(-7); d_nm.zero_()
            torch.cuda.synchronize()
            fr.search(db, B, d_match.data_ptr(), d_nm.data_ptr(), 0.75, True, st)
            stream.synchronize()
        finally:
            pkg.orbx.debug_set_bow_form("auto")
        m = d_match.cpu().numpy(); nm = d_nm.cpu().numpy()
        total = 0
        for i in range(B):
            for j in range(len(kfs)):
                exp, en = expect[i][j]
                assert nm[i, j] == en, (form, i, j, int(nm[i, j]), en)
                assert (m[i, j, :n[i]] == exp).all(), (form, i, j)
                total += int(nm[i, j])
        assert total == total_exp and total > 0 and (nm[0] == 0).all(), (form, total)
