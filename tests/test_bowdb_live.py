"""The live BowDatabase (orbx_bowdb_create_live and the seven calls behind it, k_bowdb_pack in orb-slam2_amd/csrc/orbx_bow.hip): keyframes
enter device to device, leave, and change their map-point flags while the set is searched.

What is checked: the searched form of a slot against a numpy restatement of feat_pack(..., drop_unflagged = true), array for array; every
search form on a live set against the immutable BowDatabase of the same keyframes, byte for byte over sentinel-filled buffers (-7 rows and
lists, -9 counts), and against the CPU oracle's SearchByBoW; slot reuse after erase; new flags through one set_flags call and back; the
documented use of two streams; and every refusal, after which the set must be what it was.

The scene restates the recipe of test_bow_candidates.synthetic (120 prototypes, B = 4, CAP = 384, frame counts 384 / 0 / 257 / 300, keyframes
that are shuffled bit-flipped views of the frames, one keyframe without any flag) with its LISTS / NCAND; only keyframe 7 views another frame
(257 features instead of 384), so that it is smaller than keyframe 3, whose slot it takes over in the reuse test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tools import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_CAPACITY = -1, -2
B, CAP, NKF, STRIDE = 4, 384, 11, 5
COUNTS = [384, 0, 257, 300]            # a full slot, an empty one, one past a 256-thread stride, an ordinary one
KF_BASE = [0, 3, 2, 0, 3, 3, 2, 2, 2, 3, 0]     # the frame a keyframe is a shuffled, bit-flipped view of
KF_NOFLAGS = 3                         # flags A: this keyframe has no map point at all
LISTS = [[10, 0, 10, 3, -1], [2, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 11, 2147483647, 4, 5]]      # of the candidate tests: ids are indices
NCAND = [5, 1, 0, 9]
KF_NODE_B, KF_ZERO_B, KF_RANDOM_B = 0, 2, (1, 4, 10)     # flags B: one node of keyframe 0 unflagged, keyframe 2 all-zero, three drawn afresh
FORMS = ("dense", "compact", "compact8", "cand dense", "cand compact")
WIDTH = {"dense": CAP, "compact": 2 * CAP, "compact8": 16, "cand dense": CAP, "cand compact": 2 * CAP}
NEW_SYMBOLS = {"orbx_bowdb_create_live": 5, "orbx_bowdb_add_from_frames": 6, "orbx_bowdb_add": 4, "orbx_bowdb_erase": 3, "orbx_bowdb_set_flags": 5,
               "orbx_bowdb_live_count": 1, "orbx_bowdb_ids": 3, "orbx_bowdb_read_keyframe": 12}


def slot_keyframes(lists, ncand, kf_of_id, n_ids):
    """the keyframe every slot of the candidate lists searches, or -1 (include/orbx.h); kf_of_id = dict or None (an id is the index)"""
    out = np.full((len(lists), STRIDE), -1, np.int64)
    for b, ids in enumerate(lists):
        for j in range(min(max(ncand[b], 0), STRIDE)):
            if 0 <= ids[j] < n_ids:
                out[b, j] = ids[j] if kf_of_id is None else kf_of_id.get(ids[j], -1)
    return out


def synthetic(oracle):
    """frames and keyframes of bit-flipped copies of 120 prototype descriptors, so that matches exist; FeatureVectors by the oracle; the
    keyframes carry flags A, data["flagB"] the second set"""
    rng = np.random.Generator(np.random.PCG64(7301))
    proto = rng.integers(0, 256, (120, 32), dtype=np.uint8)
    par, leaf, nd, w = synth.vocab_tree(7302, 10, 4, stop_frac=0.02, data=proto)
    ovoc = oracle.Vocabulary(10, 4, par, leaf, nd, w)

    def featset(desc, flag, angle):
        if len(desc) == 0:
            return dict(desc=np.zeros((0, 32), np.uint8), node_id=np.zeros(0, np.uint32), node_off=np.zeros(1, np.int32), feat=np.zeros(0, np.uint32),
                        flag=flag, angle=angle)
        t = ovoc.transform(desc, 2)
        return dict(desc=desc, node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"], flag=flag, angle=angle)
    desc = np.zeros((B, CAP, 32), np.uint8); angle = np.zeros((B, CAP), np.float32)
    frames = []
    for b in range(B):
        n = COUNTS[b]
        desc[b, :n] = synth.flip_bits(rng, proto[rng.integers(0, len(proto), n)], 0.06)
        angle[b, :n] = rng.uniform(0, 360, n).astype(np.float32)
        frames.append(featset(desc[b, :n].copy(), np.zeros(n, np.uint8), angle[b, :n].copy()))
    kfs = []
    for k in range(NKF):
        base = frames[KF_BASE[k]]
        n = len(base["desc"])
        perm = rng.permutation(n)
        dk = synth.flip_bits(rng, base["desc"], 0.07)[perm]
        ang = ((base["angle"] + rng.normal(0, 4, n)) % 360).astype(np.float32)[perm]       # a common rotation plus jitter: the histogram has work to do
        flag = np.zeros(n, np.uint8) if k == KF_NOFLAGS else (rng.random(n) < 0.7).astype(np.uint8)
        kfs.append(featset(dk, flag, ang))
    flag_b = [k["flag"].copy() for k in kfs]
    for k in KF_RANDOM_B:
        flag_b[k] = (rng.random(len(flag_b[k])) < 0.5).astype(np.uint8)
    kf = kfs[KF_NODE_B]                                             # the node with most flagged features loses them all
    per_node = [int(kf["flag"][kf["feat"][kf["node_off"][i]:kf["node_off"][i + 1]]].sum()) for i in range(len(kf["node_id"]))]
    node_b = int(np.argmax(per_node))
    flag_b[KF_NODE_B][kf["feat"][kf["node_off"][node_b]:kf["node_off"][node_b + 1]]] = 0
    flag_b[KF_ZERO_B][:] = 0
    return dict(par=par, leaf=leaf, nd=nd, w=w, desc=desc, angle=angle, frames=frames, kfs=kfs, flagB=flag_b, node_b=node_b)


def pack_model(kf, flag=None):
    """the searched form of a keyframe: feat_pack(..., drop_unflagged = true) of orbx_bow.hip restated.  flag[n]; node_off / feat keep only
    flagged features, order preserved, a node without survivor an empty range; sdesc = descriptors in filtered list order; sflag = 1"""
    n, nn = len(kf["desc"]), len(kf["node_id"])
    flag = np.ones(n, np.uint8) if flag is None else np.asarray(flag, np.uint8)
    off, feat = [0], []
    for i in range(nn):
        for j in range(int(kf["node_off"][i]), int(kf["node_off"][i + 1])):
            if flag[kf["feat"][j]]:
                feat.append(int(kf["feat"][j]))
        off.append(len(feat))
    feat = np.array(feat, np.uint32)
    return dict(n=n, nnodes=nn, node_id=np.asarray(kf["node_id"], np.uint32), node_off=np.array(off, np.int32), feat=feat, flag=flag,
                angle=np.asarray(kf["angle"], np.float32), desc=np.asarray(kf["desc"], np.uint8).reshape(n, 32),
                sdesc=np.asarray(kf["desc"], np.uint8).reshape(n, 32)[feat.astype(np.int64)], sflag=np.ones(len(feat), np.uint8))


def assert_packed(got, model, what):
    assert got["n"] == model["n"] and got["nnodes"] == model["nnodes"], (what, got["n"], got["nnodes"])
    for key in ("node_id", "node_off", "feat", "flag", "angle", "desc", "sdesc", "sflag"):
        assert got[key].shape == model[key].shape and got[key].tobytes() == model[key].tobytes(), (what, key)


def oracle_table(oracle, data, flags):
    """{(b, kf): (row, count)} of SearchByBoW(keyframe kf under `flags`, frame b), every pair"""
    return {(b, k): oracle.search_by_bow_kf_f(dict(data["kfs"][k], flag=flags[k]), data["frames"][b], 0.75, True) for b in range(B) for k in range(NKF)}


@pytest.fixture(scope="module")
def data(oracle):
    d = synthetic(oracle)
    d["flagA"] = [k["flag"] for k in d["kfs"]]
    d["expA"] = oracle_table(oracle, d, d["flagA"])
    d["expB"] = oracle_table(oracle, d, d["flagB"])
    return d


def test_symbols_declared_exported_and_mirrored(pkg):
    import __graft_entry__ as ge
    ge.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbx.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.lib_path())
    vp, i = C.c_void_p, C.c_int
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/orbx.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(raw, name), f"{name} is not exported"
        at = getattr(pkg.lib(), name).argtypes
        assert at is not None and len(at) == nargs, name
    at = {name: getattr(pkg.lib(), name).argtypes for name in NEW_SYMBOLS}
    assert list(at["orbx_bowdb_create_live"][:4]) == [i, i, i, i]
    assert list(at["orbx_bowdb_add_from_frames"]) == [vp, i, vp, i, vp, vp]
    assert at["orbx_bowdb_add"][0] is vp and at["orbx_bowdb_add"][1] is i and at["orbx_bowdb_add"][3] is vp
    assert list(at["orbx_bowdb_erase"]) == [vp, i, vp]
    assert at["orbx_bowdb_set_flags"][0] is vp and at["orbx_bowdb_set_flags"][2] is i and at["orbx_bowdb_set_flags"][4] is vp
    assert list(at["orbx_bowdb_ids"]) == [vp, vp, i]
    assert at["orbx_bowdb_read_keyframe"][1] is i and all(a is vp for a in at["orbx_bowdb_read_keyframe"][4:])
    for meth in ("live", "add_from_frames", "add", "erase", "set_flags", "ids", "live_count", "read_keyframe"):
        assert callable(getattr(pkg.BowDatabase, meth)), meth


def test_scene_is_not_vacuous(oracle, data):
    """checks the fixture, not the feature, on the oracle alone: the searched slots of the candidate lists on frames that have features average
    at least 20 matches; the oracle's row differs between flags A and B for at least three searched slots; B differs from A on at least three
    keyframes; the packed model has an empty node range where B unflags a whole node; keyframe 7 is smaller than keyframe 3"""
    kf = slot_keyframes(LISTS, NCAND, None, NKF)
    assert kf.tolist() == [[10, 0, 10, 3, -1], [2, -1, -1, -1, -1], [-1] * 5, [1, -1, -1, 4, 5]]
    slots = [(b, int(k)) for b in range(B) for k in kf[b] if k >= 0]
    cnt = [data["expA"][s][1] for s in slots if COUNTS[s[0]] > 0]
    assert len(cnt) == 7 and np.mean(cnt) >= 20, cnt
    assert max(cnt) > 8                                           # a list capacity of 8 cuts at least one list
    differ = {s for s in slots if data["expA"][s][0].tobytes() != data["expB"][s][0].tobytes()}
    assert len(differ) >= 3, differ
    changed = [k for k in range(NKF) if data["flagA"][k].tobytes() != data["flagB"][k].tobytes()]
    assert len(changed) >= 3 and KF_NODE_B in changed and KF_ZERO_B in changed
    assert not data["flagA"][KF_NOFLAGS].any() and not data["flagB"][KF_ZERO_B].any() and data["flagA"][KF_ZERO_B].any()
    a, b_ = pack_model(data["kfs"][KF_NODE_B], data["flagA"][KF_NODE_B]), pack_model(data["kfs"][KF_NODE_B], data["flagB"][KF_NODE_B])
    nb = data["node_b"]
    assert a["node_off"][nb + 1] > a["node_off"][nb] and b_["node_off"][nb + 1] == b_["node_off"][nb]
    assert 0 < len(b_["feat"]) < len(a["feat"]) and (np.diff(b_["node_off"]) > 0).any()
    assert len(data["kfs"][7]["desc"]) < len(data["kfs"][3]["desc"])


# ------------------------------------------------------------------------------------------ GPU

class Scene:
    """the frames resident in one BowFrames, the keyframes' descriptors and angles through a second one (so that they can be added from
    frames), the flag sets on the device, and the five searches"""

    def __init__(self, pkg, data):
        import torch
        self.torch, self.pkg, self.data = torch, pkg, data
        self.stream = torch.cuda.Stream(); self.st = self.stream.cuda_stream
        self.voc = pkg.ORBVocabulary(10, 4, data["par"], data["leaf"], data["nd"], data["w"])
        kps = np.zeros((B, CAP, 7), np.float32)
        kps[:, :, 3] = data["angle"]                                  # cv::KeyPoint.angle, the only field the transform reads
        self.fr, self._keep_f = self._frames(kps, data["desc"], COUNTS)
        kkps = np.zeros((NKF, CAP, 7), np.float32); kdesc = np.zeros((NKF, CAP, 32), np.uint8)
        self.kf_n = [len(k["desc"]) for k in data["kfs"]]
        for k, kf in enumerate(data["kfs"]):
            kkps[k, :self.kf_n[k], 3] = kf["angle"]; kdesc[k, :self.kf_n[k]] = kf["desc"]
        self.kfr, self._keep_k = self._frames(kkps, kdesc, self.kf_n)
        self.d_flags = {}
        for name, flags in (("A", data["flagA"]), ("B", data["flagB"]), ("zero", [np.zeros(n, np.uint8) for n in self.kf_n])):
            h = np.full((NKF, CAP), 1, np.uint8)                      # (beyond a keyframe's n the bytes must not matter)
            for k in range(NKF):
                h[k, :self.kf_n[k]] = flags[k]
            self.d_flags[name] = torch.from_numpy(h).cuda()
        self.d_lists = torch.tensor(LISTS, dtype=torch.int32, device="cuda"); self.d_ncand = torch.tensor(NCAND, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def _frames(self, kps, desc, counts):
        torch = self.torch
        t = (torch.from_numpy(kps).cuda(), torch.from_numpy(desc).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"))
        fr = self.pkg.BowFrames(len(counts), CAP)
        torch.cuda.synchronize()
        fr.transform(self.voc, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(counts), 2, self.st)
        self.stream.synchronize()
        return fr, t

    def live(self, flags="A", keyframes=range(NKF), ids=None, max_kf=NKF, max_ids=NKF):
        """a live set with `keyframes` added from the resident frames in that order, under `ids` (default: their indices)"""
        db = self.pkg.BowDatabase.live(max_kf, CAP, max_ids)
        for pos, k in enumerate(keyframes):
            self.add(db, k if ids is None else ids[pos], k, flags)
        return db

    def add(self, db, id, k, flags="A", stream=None):
        d_flag = None if flags is None else self.d_flags[flags][k].data_ptr()
        db.add_from_frames(id, self.kfr, k, d_flag, self.st if stream is None else stream)

    def search(self, db, form, lists=None, ncand=None, stream=None, sync=True):
        """one of FORMS on `db` -> (rows or lists, counts) as numpy, over sentinel-filled buffers"""
        torch = self.torch
        st = self.st if stream is None else stream
        cand = form.startswith("cand")
        nrows = STRIDE if cand else db.size()
        m = torch.full((B, nrows, WIDTH[form]), -7, dtype=torch.int32, device="cuda"); nm = torch.full((B, nrows), -9, dtype=torch.int32, device="cuda")
        d_l = self.d_lists if lists is None else torch.tensor(lists, dtype=torch.int32, device="cuda")
        d_n = self.d_ncand if ncand is None else torch.tensor(ncand, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if form == "dense":
            self.fr.search(db, B, m.data_ptr(), nm.data_ptr(), 0.75, True, st)
        elif form in ("compact", "compact8"):
            self.fr.search_compact(db, B, m.data_ptr(), WIDTH[form] // 2, nm.data_ptr(), 0.75, True, st)
        elif form == "cand dense":
            self.fr.search_candidates(db, B, d_l.data_ptr(), STRIDE, d_n.data_ptr(), m.data_ptr(), nm.data_ptr(), 0.75, True, stream=st)
        else:
            self.fr.search_candidates_compact(db, B, d_l.data_ptr(), STRIDE, d_n.data_ptr(), m.data_ptr(), WIDTH[form] // 2, nm.data_ptr(), 0.75, True, stream=st)
        if not sync:
            return m, nm, (d_l, d_n)
        torch.cuda.synchronize()
        return m.cpu().numpy(), nm.cpu().numpy()

    def five(self, db):
        return {form: self.search(db, form) for form in FORMS}


@pytest.fixture(scope="module")
def scene(pkg, data):
    return Scene(pkg, data)


@pytest.fixture(scope="module")
def immutable(pkg, data, scene):
    """the five searches on BowDatabase(kfs) under flags A and B, computed once"""
    out = {}
    for name in ("A", "B"):
        db = pkg.BowDatabase([dict(k, flag=data["flag" + name][i]) for i, k in enumerate(data["kfs"])])
        out[name] = scene.five(db)
    return out


def check_rows(form, got, kf_of, expect):
    """rows of a search against the oracle: kf_of[b][j] = the keyframe behind row j of frame b, -1 = a slot that is not searched (count -1, row
    untouched), -2 = an empty slot of an all-keyframes search (a keyframe without features: count 0, nothing matched)"""
    m, nm = got
    assert m.shape[1] == len(kf_of[0]), (form, m.shape)
    searched = 0
    for b in range(B):
        n = COUNTS[b]
        for j, kf in enumerate(kf_of[b]):
            kf = int(kf)
            if kf == -1:
                assert nm[b, j] == -1 and (m[b, j] == -7).all(), (form, b, j)
                continue
            exp, en = (np.full(n, -1, np.int32), 0) if kf == -2 else expect[(b, kf)]
            assert nm[b, j] == en, (form, b, j, kf, int(nm[b, j]), en)
            if form in ("dense", "cand dense"):
                assert (m[b, j, :n] == exp).all() and (m[b, j, n:] == -7).all(), (form, b, j, kf)
            else:
                slots = np.nonzero(exp >= 0)[0]
                keep = min(en, m.shape[2] // 2)
                lst = m[b, j].reshape(-1, 2)
                assert (lst[:keep, 0] == slots[:keep]).all() and (lst[:keep, 1] == exp[slots[:keep]]).all() and (lst[keep:] == -7).all(), (form, b, j, kf)
            searched += kf >= 0
    return searched


def check_five(got, expect, ref=None):
    """the five searches of a set holding keyframes 0..NKF-1 under ids equal to the indices: the oracle for every searched slot, and -- where
    given -- the immutable set's buffers byte for byte"""
    every = [list(range(NKF))] * B
    cand = slot_keyframes(LISTS, NCAND, None, NKF)
    for form in FORMS:
        n = check_rows(form, got[form], cand if form.startswith("cand") else every, expect)
        assert n == (8 if form.startswith("cand") else B * NKF), (form, n)      # (8: the seven of the fixture test and the one on the featureless frame)
        if ref is not None:
            assert got[form][0].tobytes() == ref[form][0].tobytes() and got[form][1].tobytes() == ref[form][1].tobytes(), form


@pytest.mark.gpu
@pytest.mark.parametrize("flags", ["A", None, "zero"])
def test_packed_form(pkg, data, scene, flags):
    """add_from_frames of every keyframe with d_flag = A, NULL and all-zero: read_keyframe equals the numpy model array for array, and
    orbx_bowdb_add of the same keyframe from its host feature set reads back identical"""
    db = scene.live(flags)
    host = pkg.BowDatabase.live(NKF, CAP, NKF)
    for k, kf in enumerate(data["kfs"]):
        fl = None if flags is None else (data["flagA"][k] if flags == "A" else np.zeros(len(kf["desc"]), np.uint8))
        model = pack_model(kf, fl)
        got = db.read_keyframe(k)
        assert_packed(got, model, ("from frames", flags, k))
        host.add(k, dict(kf, flag=model["flag"]))
        assert_packed(host.read_keyframe(k), got, ("from the host", flags, k))
    assert db.live_count() == host.live_count() == NKF and db.ids().tolist() == host.ids().tolist() == list(range(NKF))


@pytest.mark.gpu
def test_same_answers_as_the_immutable_set(pkg, data, scene, immutable):
    """a live set with keyframes 0..NKF-1 added in order under their indices against BowDatabase(kfs): the all-keyframes dense and compact
    searches, the compact one with cap_pairs = 8, and the candidate search in both forms over LISTS / NCAND, byte-identical over the whole
    output buffers; the searched slots are the oracle's SearchByBoW"""
    db = scene.live("A")
    assert db.size() == NKF
    check_five(scene.five(db), data["expA"], immutable["A"])


@pytest.mark.gpu
def test_erase_and_slot_reuse(pkg, oracle, data, scene):
    db = scene.live("A", keyframes=range(6), ids=[3, 7, 1, 9, 12, 4], max_kf=6, max_ids=16)
    assert db.ids().tolist() == [3, 7, 1, 9, 12, 4] and db.live_count() == 6
    with pytest.raises(pkg.OrbxError) as ei:
        scene.add(db, 13, 6)
    assert ei.value.code == E_CAPACITY and db.ids().tolist() == [3, 7, 1, 9, 12, 4] and db.live_count() == 6
    db.erase(7, scene.st); db.erase(9, scene.st)
    assert db.ids().tolist() == [3, -1, 1, -1, 12, 4] and db.live_count() == 4 and db.size() == 6
    scene.add(db, 13, 6)                                          # the lowest free slot first
    assert db.ids().tolist() == [3, 13, 1, -1, 12, 4]
    scene.add(db, 15, 7)                                          # 257 features where keyframe 3 had 384: a stale tail would show
    assert db.ids().tolist() == [3, 13, 1, 15, 12, 4] and db.live_count() == 6
    assert_packed(db.read_keyframe(15), pack_model(data["kfs"][7], data["flagA"][7]), "keyframe 7 in the slot of keyframe 3")
    kf_of_id = {3: 0, 13: 6, 1: 2, 15: 7, 12: 4, 4: 5}
    # live ids, the erased 7 and 9, the never-added 0 and 2, and -1 / 16 / 2^31 - 1 outside [0, max_ids); frame 1 has no features
    lists = [[3, 13, 7, 15, 16], [1, 9, 0, 0, 0], [12, 4, -1, 2, 13], [15, 3, 2147483647, 9, 4]]
    ncand = [5, 2, 5, 5]
    kf_of = slot_keyframes(lists, ncand, kf_of_id, 16)
    assert kf_of.tolist() == [[0, 6, -1, 7, -1], [2, -1, -1, -1, -1], [4, 5, -1, -1, 6], [7, 0, -1, -1, 5]]
    for form in ("cand dense", "cand compact"):
        assert check_rows(form, scene.search(db, form, lists, ncand), kf_of, data["expA"]) == 10
    db.erase(12, scene.st)                                        # one more, not added again: its slot reads as a featureless keyframe
    assert db.live_count() == 5 and db.ids().tolist() == [3, 13, 1, 15, -1, 4] and db.size() == 6
    every = [[0, 6, 2, 7, -2, 5]] * B
    for form in ("dense", "compact", "compact8"):
        assert check_rows(form, scene.search(db, form), every, data["expA"]) == 5 * B
    kf_of[2, 0] = -1                                              # and the candidate search no longer finds id 12
    assert check_rows("cand compact", scene.search(db, "cand compact", lists, ncand), kf_of, data["expA"]) == 9
    scene.add(db, 7, 1)                                           # an erased id may be added again
    assert db.ids().tolist() == [3, 13, 1, 15, 7, 4]
    assert_packed(db.read_keyframe(7), pack_model(data["kfs"][1], data["flagA"][1]), "id 7 again")


@pytest.mark.gpu
def test_reflag(pkg, data, scene, immutable):
    """one set_flags call for the keyframes whose flags differ, A -> B: the packed form is the model's for B, the searches are those of an
    immutable set built with B and the oracle's; back to A everything is restored byte for byte (the master is kept)"""
    db = scene.live("A")
    before = scene.five(db)
    packed = [db.read_keyframe(k) for k in range(NKF)]
    changed = [k for k in range(NKF) if data["flagA"][k].tobytes() != data["flagB"][k].tobytes()]
    assert len(changed) >= 3
    db.set_flags(changed, [data["flagB"][k] for k in changed], scene.st)
    for k in range(NKF):
        assert_packed(db.read_keyframe(k), pack_model(data["kfs"][k], data["flagB"][k]), ("B", k))
    check_five(scene.five(db), data["expB"], immutable["B"])
    db.set_flags(changed, [data["flagA"][k] for k in changed], scene.st)
    for k in range(NKF):
        assert_packed(db.read_keyframe(k), packed[k], ("A again", k))
    check_five(scene.five(db), data["expA"], before)


@pytest.mark.gpu
def test_two_streams(pkg, data, scene):
    """the documented usage: add on one stream, search the candidates on another with no host synchronisation between, then erase and add
    another keyframe into the same slot on the first stream.  The search sees the first keyframe, a later one the second.  (That the wait /
    record pair is there is for the review of orbx_bow.hip: without it this test may still pass.)"""
    torch = scene.torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    db = pkg.BowDatabase.live(2, CAP, 8)
    lists = [[5, 0, 0, 0, 0]] * B
    ncand = [1] * B
    torch.cuda.synchronize()
    scene.add(db, 5, 0, "A", s1.cuda_stream)
    m, nm, keep = scene.search(db, "cand compact", lists, ncand, stream=s2.cuda_stream, sync=False)
    db.erase(5, s1.cuda_stream)
    scene.add(db, 5, 10, "A", s1.cuda_stream)
    torch.cuda.synchronize()
    assert db.ids().tolist() == [5]
    kf_of = np.full((B, STRIDE), -1)
    kf_of[:, 0] = 0
    assert check_rows("cand compact", (m.cpu().numpy(), nm.cpu().numpy()), kf_of, data["expA"]) == B
    kf_of[:, 0] = 10
    assert check_rows("cand compact", scene.search(db, "cand compact", lists, ncand, stream=s2.cuda_stream), kf_of, data["expA"]) == B


@pytest.mark.gpu
def test_refusals(pkg, data, scene, immutable):
    """every ORBX_E_INVALID / ORBX_E_CAPACITY case of include/orbx.h; after each the set is what it was: ids() and one search are compared"""
    import torch
    L = pkg.lib()
    db = scene.live("A", keyframes=range(3), ids=[4, 0, 6], max_kf=3, max_ids=8)
    frozen = pkg.BowDatabase(data["kfs"][:2])
    lists, ncand = [[4, 0, 6, 1, 7]] * B, [5] * B
    base_ids = db.ids().tolist()
    base = scene.search(db, "cand compact", lists, ncand)
    kf_of = np.array([[0, 1, 2, -1, -1]] * B)
    assert check_rows("cand compact", base, kf_of, data["expA"]) == 3 * B
    fs, keep = pkg.make_featset(data["kfs"][5])
    big = pkg.BowDatabase.live(2, 100, 4)                         # slots too small for any keyframe of the scene
    bad_fs, keep2 = pkg.make_featset(dict(data["kfs"][5], node_off=data["kfs"][5]["node_off"] + 1))
    other_cap = pkg.BowFrames(2, CAP + 1)                         # untransformed: refused before anything reads it
    n, nn = C.c_int(), C.c_int()
    idbuf = np.zeros(8, np.int32)
    one_id = np.array([4], np.int32); gone_id = np.array([5], np.int32); twice = np.array([4, 4], np.int32)
    fl = np.ones(CAP, np.uint8)
    p1 = (C.c_void_p * 2)(fl.ctypes.data, fl.ctypes.data)
    none1 = (C.c_void_p * 1)(None)
    d_flag = scene.d_flags["A"][5].data_ptr()
    h, hf, kfr, st = db._h, frozen._h, scene.kfr._h, scene.st
    rk = lambda d, i: L.orbx_bowdb_read_keyframe(d, i, C.byref(n), C.byref(nn), None, None, None, None, None, None, None, None)
    cases = {
        # NULL arguments
        "create: NULL out": (lambda: L.orbx_bowdb_create_live(0, 3, CAP, 8, None), E_INVALID),
        "create: max_kf 0": (lambda: L.orbx_bowdb_create_live(0, 0, CAP, 8, C.byref(C.c_void_p())), E_INVALID),
        "create: cap above 8192": (lambda: L.orbx_bowdb_create_live(0, 3, 8193, 8, C.byref(C.c_void_p())), E_INVALID),
        "create: max_ids 0": (lambda: L.orbx_bowdb_create_live(0, 3, CAP, 0, C.byref(C.c_void_p())), E_INVALID),
        "add_from_frames: NULL db": (lambda: L.orbx_bowdb_add_from_frames(None, 1, kfr, 5, d_flag, st), E_INVALID),
        "add_from_frames: NULL frames": (lambda: L.orbx_bowdb_add_from_frames(h, 1, None, 5, d_flag, st), E_INVALID),
        "add: NULL db": (lambda: L.orbx_bowdb_add(None, 1, C.byref(fs), st), E_INVALID),
        "add: NULL feature set": (lambda: L.orbx_bowdb_add(h, 1, None, st), E_INVALID),
        "erase: NULL db": (lambda: L.orbx_bowdb_erase(None, 4, st), E_INVALID),
        "set_flags: NULL db": (lambda: L.orbx_bowdb_set_flags(None, one_id.ctypes.data, 1, p1, st), E_INVALID),
        "set_flags: NULL ids": (lambda: L.orbx_bowdb_set_flags(h, None, 1, p1, st), E_INVALID),
        "set_flags: NULL flags": (lambda: L.orbx_bowdb_set_flags(h, one_id.ctypes.data, 1, None, st), E_INVALID),
        "set_flags: a NULL flag array": (lambda: L.orbx_bowdb_set_flags(h, one_id.ctypes.data, 1, none1, st), E_INVALID),
        "live_count: NULL db": (lambda: L.orbx_bowdb_live_count(None), E_INVALID),
        "ids: NULL db": (lambda: L.orbx_bowdb_ids(None, idbuf.ctypes.data, 8), E_INVALID),
        "ids: NULL array": (lambda: L.orbx_bowdb_ids(h, None, 8), E_INVALID),
        "read_keyframe: NULL db": (lambda: rk(None, 4), E_INVALID),
        # an immutable set handed to a live-only call
        "add_from_frames: immutable": (lambda: L.orbx_bowdb_add_from_frames(hf, 1, kfr, 5, d_flag, st), E_INVALID),
        "add: immutable": (lambda: L.orbx_bowdb_add(hf, 1, C.byref(fs), st), E_INVALID),
        "erase: immutable": (lambda: L.orbx_bowdb_erase(hf, 0, st), E_INVALID),
        "set_flags: immutable": (lambda: L.orbx_bowdb_set_flags(hf, one_id.ctypes.data, 1, p1, st), E_INVALID),
        "live_count: immutable": (lambda: L.orbx_bowdb_live_count(hf), E_INVALID),
        "ids: immutable": (lambda: L.orbx_bowdb_ids(hf, idbuf.ctypes.data, 8), E_INVALID),
        "read_keyframe: immutable": (lambda: rk(hf, 0), E_INVALID),
        # frames, index, id
        "add_from_frames: another cap": (lambda: L.orbx_bowdb_add_from_frames(h, 1, other_cap._h, 0, None, st), E_INVALID),
        "add_from_frames: index -1": (lambda: L.orbx_bowdb_add_from_frames(h, 1, kfr, -1, d_flag, st), E_INVALID),
        "add_from_frames: index = batch": (lambda: L.orbx_bowdb_add_from_frames(h, 1, kfr, NKF, d_flag, st), E_INVALID),
        "add_from_frames: id -1": (lambda: L.orbx_bowdb_add_from_frames(h, -1, kfr, 5, d_flag, st), E_INVALID),
        "add_from_frames: id = max_ids": (lambda: L.orbx_bowdb_add_from_frames(h, 8, kfr, 5, d_flag, st), E_INVALID),
        "add_from_frames: id already live": (lambda: L.orbx_bowdb_add_from_frames(h, 4, kfr, 5, d_flag, st), E_INVALID),
        "add: id -1": (lambda: L.orbx_bowdb_add(h, -1, C.byref(fs), st), E_INVALID),
        "add: id = max_ids": (lambda: L.orbx_bowdb_add(h, 8, C.byref(fs), st), E_INVALID),
        "add: id already live": (lambda: L.orbx_bowdb_add(h, 6, C.byref(fs), st), E_INVALID),
        "add: malformed feature set": (lambda: L.orbx_bowdb_add(h, 1, C.byref(bad_fs), st), E_INVALID),
        "add: more features than cap": (lambda: L.orbx_bowdb_add(big._h, 1, C.byref(fs), st), E_INVALID),
        "erase: id not live": (lambda: L.orbx_bowdb_erase(h, 5, st), E_INVALID),
        "erase: id -1": (lambda: L.orbx_bowdb_erase(h, -1, st), E_INVALID),
        "erase: id = max_ids": (lambda: L.orbx_bowdb_erase(h, 8, st), E_INVALID),
        "set_flags: id not live": (lambda: L.orbx_bowdb_set_flags(h, gone_id.ctypes.data, 1, p1, st), E_INVALID),
        "set_flags: an id twice": (lambda: L.orbx_bowdb_set_flags(h, twice.ctypes.data, 2, p1, st), E_INVALID),
        "set_flags: n -1": (lambda: L.orbx_bowdb_set_flags(h, one_id.ctypes.data, -1, p1, st), E_INVALID),
        "read_keyframe: id not live": (lambda: rk(h, 5), E_INVALID),
        "read_keyframe: id = max_ids": (lambda: rk(h, 8), E_INVALID),
        "ids: array too small": (lambda: L.orbx_bowdb_ids(h, idbuf.ctypes.data, 2), E_CAPACITY),
        # no free slot
        "add_from_frames: full": (lambda: L.orbx_bowdb_add_from_frames(h, 1, kfr, 5, d_flag, st), E_CAPACITY),
        "add: full": (lambda: L.orbx_bowdb_add(h, 1, C.byref(fs), st), E_CAPACITY),
    }
    if L.orbx_device_count() > 1:                                 # frames of another device
        other = pkg.BowFrames(2, CAP, device=1)
        cases["add_from_frames: another device"] = (lambda: L.orbx_bowdb_add_from_frames(h, 1, other._h, 0, None, st), E_INVALID)
    d_map = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_l = torch.tensor(lists, dtype=torch.int32, device="cuda"); d_n = torch.tensor(ncand, dtype=torch.int32, device="cuda")
    m = torch.full((B, STRIDE, 2 * CAP), -7, dtype=torch.int32, device="cuda"); nm = torch.full((B, STRIDE), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cases["candidates: an explicit map with a live set"] = (lambda: L.orbx_bowdb_search_candidates_device(
        h, scene.fr._h, B, d_l.data_ptr(), STRIDE, d_n.data_ptr(), d_map.data_ptr(), 8, 0.75, 1, m.data_ptr(), nm.data_ptr(), st), E_INVALID)
    cases["candidates, compact: an explicit map with a live set"] = (lambda: L.orbx_bowdb_search_candidates_device_compact(
        h, scene.fr._h, B, d_l.data_ptr(), STRIDE, d_n.data_ptr(), d_map.data_ptr(), 8, 0.75, 1, m.data_ptr(), CAP, nm.data_ptr(), st), E_INVALID)
    for name, (call, code) in cases.items():
        assert call() == code, name
        assert db.ids().tolist() == base_ids and db.live_count() == 3 and db.size() == 3, name
        got = scene.search(db, "cand compact", lists, ncand)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), name
    assert (m == -7).all().item() and (nm == -9).all().item()
    assert big.live_count() == 0 and big.size() == 0
    for k in range(3):                                            # and the keyframes themselves
        assert_packed(db.read_keyframe(base_ids[k]), pack_model(data["kfs"][k], data["flagA"][k]), ("after the refusals", k))
    with pytest.raises(pkg.OrbxError) as ei:                      # and through the mirror
        db.erase(5)
    assert ei.value.code == E_INVALID
    with pytest.raises(pkg.OrbxError) as ei:
        db.set_flags([4], [np.ones(3, np.uint8)])                 # a flag array of the wrong length never reaches the C entry
    assert ei.value.code == E_INVALID
